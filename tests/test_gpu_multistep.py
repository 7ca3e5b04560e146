"""The fused few-step samplers of the probability-flow ODE, DPM-Solver++(2M) and DDIM (dmip_multistep_sample;
solver="dpm2m" / "ddim", grid=, t_end=, x0=) against their numpy restatement (tests/multistep_ref.py). Needs an MI355X:
`pytest -m gpu`.

Bound 1 is the project's own for ten network evaluations of these engines (tests/heun_ref.py BOUND): 1e-4 max(1, |ref|)
for exact f32 and 1e-3 max(1, |ref|) for fp32x3, against the f64 restatement; the runs here make six. The f32 rounding
order of the table-driven update itself stays below a quarter of the f32 bound (tests/test_multistep_host.py).
"""
import functools

import numpy as np
import pytest
import torch

import accuracy_cases as AC
import heun_ref as HR
import multistep_ref as MR
import oracle as O
import sde_cases as SC
from conftest import GOLDEN, state_from_npz

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
S6 = MR.PARITY_STEPS


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def _raw(t):
    return t.cpu().numpy().view(np.uint32)


def _bound(prec, ref):
    return HR.BOUND[prec] * max(1.0, float(np.abs(ref).max()))


def _mode(dmip, kind):
    return dmip._lib.DMIP_SAMPLER_CDE if kind == "cde" else dmip._lib.DMIP_SAMPLER_POSTERIOR


def _sample(dmip, m, y, n, S, solver, fused=True, **kw):
    """m.sample_device(solver=) for one y -> (n, xdim) numpy; the launch counters show the path taken."""
    calls = dmip._lib.calls
    before = calls["multistep_sample"], calls["mlp_forward"], calls["ode_sample"], calls["em_sample_lmbd"]
    out = m.sample_device(torch.as_tensor(np.asarray(y, np.float32)).to(DEV), n, S, solver=solver, **kw)
    dmip._lib.device_status(torch.device(DEV))
    assert (calls["ode_sample"], calls["em_sample_lmbd"]) == before[2:]
    if fused:
        assert calls["multistep_sample"] == before[0] + 1 and calls["mlp_forward"] == before[1]
    else:
        assert calls["multistep_sample"] == before[0] and calls["mlp_forward"] > before[1]
    return out[0].cpu().numpy()


# ------------------------------------------------------------------------------ 1. parity, x0 injected
@functools.lru_cache(maxsize=None)
def _parity_ref(dmip, case, solver, grid):
    m, params, prior, y, x0 = HR.parity_case(dmip, *case)
    ref = MR.direct_sample(params, x0, y, S6, solver, grid, prior)
    ref.setflags(write=False)
    return m, params, prior, y, x0, ref


@pytest.mark.parametrize("solver", MR.SOLVERS)
@pytest.mark.parametrize("prec", ["fp32", "fp32x3"])
@pytest.mark.parametrize("case,grid", [(c, "logsnr") for c in HR.PARITY_CASES] + [(HR.PARITY_CASES[1], "uniform")],
                         ids=lambda v: v if isinstance(v, str) else f"{v[0]}-{v[1]}")
def test_parity_with_the_restatement(dmip, case, grid, prec, solver):
    """Random weights, three hidden layers, S = 6, x0 injected, the default VP-SDE: bound 1 against the scheme stated
    directly in float64. The fused kernel runs wherever dmip_multistep_supported says so; the exact-f32 shape it
    leaves out (width 512 with the tanh chain would spill) steps through the loop, to the same bound."""
    kind, W, xd, yd, n = case
    m, params, prior, y, x0, ref = _parity_ref(dmip, case, solver, grid)
    fused = dmip._lib.multistep_supported(W, 3, xd, yd, _mode(dmip, kind), prec)
    assert fused == (not (W == 512 and prec == "fp32"))
    out = _sample(dmip, m, y, n, S6, solver, fused=fused, x0=torch.from_numpy(x0), precision=prec, grid=grid)
    err = HR.max_err(out, ref)
    print(f"{kind} W={W} {prec} {solver} {grid}: max |kernel - f64 restatement| = {err:.3e} "
          f"(bound {_bound(prec, ref):.1e}, max |ref| {np.abs(ref).max():.3g})")
    assert np.all(np.isfinite(out)) and err < _bound(prec, ref), err


@pytest.mark.parametrize("kind", ["cde", "posterior"])
def test_shape_without_a_kernel_steps_through_the_loop(dmip, kind):
    """xdim 4 has no fused sampler: one dmip_mlp_forward launch per network and step, the same update from the same
    table, bound 1 (exact f32) against the restatement; shards of the loop's own x0 stay bit-identical."""
    torch.manual_seed(96)
    m = (dmip.CDE if kind == "cde" else dmip.PosteriorDiffusionEstimator)(4, 5, [64] * 3)
    if kind == "cde":
        params, prior = HR.params_of(m.sde.a), None
    else:
        params, prior = HR.params_of(m.sde.a.likelihood_net), HR.params_of(m.sde.a.prior_net)
    g = torch.Generator().manual_seed(5)
    y, x0 = torch.randn(5, generator=g).numpy(), torch.randn(200, 4, generator=g).numpy()
    ref = MR.direct_sample(params, x0, y, S6, "dpm2m", "logsnr", prior)
    before = dmip._lib.calls["mlp_forward"]
    out = _sample(dmip, m, y, 200, S6, "dpm2m", fused=False, x0=torch.from_numpy(x0), precision="fp32x3")
    assert dmip._lib.calls["mlp_forward"] == before + S6 * (1 if kind == "cde" else 2)
    err = HR.max_err(out, ref)
    assert np.all(np.isfinite(out)) and err < _bound("fp32", ref), err
    yt = torch.from_numpy(y).to(DEV)
    full = m.sample_device(yt, 90, 3, seed=4, solver="dpm2m")
    part = m.sample_device(yt, 50, 3, seed=4, chain_offset=40, solver="dpm2m")
    np.testing.assert_array_equal(_raw(part), _raw(full[:, 40:]))


@pytest.mark.parametrize("W,xd,yd", [(64, 2, 2), (256, 3, 23), (512, 3, 23)])
def test_silu_cde_on_exact_f32(dmip, W, xd, yd):
    """The SiLU chain has the exact-f32 CDE kernel only, whatever precision is asked for, width 512 included: bound 1
    against the float64 scheme with heun_ref's SiLU network (tests/test_gpu_heun.py pins that one to eager torch)."""
    torch.manual_seed(W + 2)
    m = dmip.CDE(xd, yd, [W] * 3)
    m.sde.a = dmip.MLP(xd + yd + 1, xd, [W] * 3, torch.nn.SiLU()).to(DEV)
    g = torch.Generator().manual_seed(9)
    y, x0 = torch.randn(yd, generator=g).numpy(), torch.randn(100, xd, generator=g).numpy()
    ref = MR.direct_sample(HR.params_of(m.sde.a), x0, y, S6, "dpm2m", "logsnr", act="silu")
    for prec in ("fp32", "fp32x3"):
        out = _sample(dmip, m, y, 100, S6, "dpm2m", x0=torch.from_numpy(x0), precision=prec)
        err = HR.max_err(out, ref)
        print(f"SiLU W={W} ({prec} asked): {err:.3e} (bound {_bound('fp32', ref):.1e})")
        assert np.all(np.isfinite(out)) and err < _bound("fp32", ref), err


# ------------------------------------------------------------------------------ 2. the f32-accuracy gate
GATE = [("cde", 64, 2, 2, 49), ("cde", 256, 3, 23, 49), ("posterior", 64, 2, 2, 49), ("posterior", 256, 3, 23, 49)]


@functools.lru_cache(maxsize=None)
def _gate_refs(dmip, case, sde, solver):
    """(params, prior, y, x0, f64 scheme, f32 restatement) of a gate case at the VP-SDE `sde`, read-only."""
    _, params, prior, y, x0 = HR.parity_case(dmip, *case)
    kw = SC.kw(sde)
    r64 = MR.direct_sample(params, x0, y, S6, solver, "logsnr", prior, **kw)
    r32 = MR.table_sample(params, x0, y, MR.table_of(dmip, solver, "logsnr", S6, **kw), prior, dtype=np.float32)
    for a in (r64, r32):
        a.setflags(write=False)
    return params, prior, y, x0, r64, r32


@pytest.mark.parametrize("prec", AC.PRECISIONS)
@pytest.mark.parametrize("case,sde", [(c, AC.M) for c in GATE] + [(GATE[0], SC.SDES["B"])],
                         ids=lambda v: v if isinstance(v, str) else f"{v[0]}-{v[1]}" if isinstance(v[0], str)
                         else "sde-%g-%g-%g" % v)
def test_f32_accuracy_gate(dmip, case, sde, prec):
    """The gate of tests/accuracy_cases.py: err(gpu) <= 8 max(err(f32 restatement), 1e-7), element-wise relative errors
    against the float64 scheme, at the mild VP-SDE (0.1, 2, 1) where the layers stay out of saturation -- CDE and
    Posterior, both precisions, S = 6 of "dpm2m" -- and one case at the non-default SDE B of tests/sde_cases.py
    (beta_min, beta_max and T all off their defaults: it enters the kernel through the table alone)."""
    kind, W, xd, yd, n = case
    params, prior, y, x0, r64, r32 = _gate_refs(dmip, case, sde, "dpm2m")
    m = SC.set_sde(dmip, HR.parity_case(dmip, *case)[0], sde)
    out = _sample(dmip, m, y, n, S6, "dpm2m", x0=torch.from_numpy(x0), precision=prec)
    e_cpu, e_gpu = AC.err(r32, r64), AC.err(out, r64)
    base = max(e_cpu, AC.FLOOR)
    print(f"{kind} W={W} {prec} sde {sde}: e_gpu = {e_gpu:.3e}, e_cpu = {e_cpu:.3e}, ratio = {e_gpu / base:.2f} "
          f"(K = {AC.K:g}), max |ref| = {np.abs(r64).max():.4g}")
    assert np.all(np.isfinite(out))
    assert e_gpu <= AC.K * base, (e_gpu, e_cpu)


# ------------------------------------------------------------------------------ 3. the history crosses a hand-over
@pytest.mark.parametrize("prec", ["fp32x3", "fp32"])
@pytest.mark.parametrize("solver", MR.SOLVERS)
def test_history_through_the_hand_over(dmip, prec, solver):
    """Width 256, 70001 chains, S = 4, internal RNG: 4376 tiles over at most 4096 waves of either engine's grid (256
    CUs, at most two 8-wave workgroups each at this width), so the balanced schedule cuts tiles between waves (the size
    of tests/test_gpu_heun.py's split run). Two runs are bitwise equal; three ragged chain_offset shards concatenate
    bitwise to the full run; and rows of the full run equal, bitwise, launches of 1000 of the same global chains, which
    hold one tile per wave and cannot split. A "dpm2m" tile resumed at step s > 0 without d_{s-1} would take that step
    with c1 d_prev missing and differ from the unsplit launch (checked once on a build that drops it: DESIGN.md 3h)."""
    n, S, seed = 70001, 4, 77
    torch.manual_seed(256 + n)
    m = dmip.CDE(3, 23, [256] * 3)
    y = torch.from_numpy(np.random.default_rng(5).uniform(0, 1, (1, 23)).astype(np.float32)).to(DEV)
    kw = dict(seed=seed, precision=prec, solver=solver)
    before = dmip._lib.calls["multistep_sample"]
    full = m.sample_device(y, n, S, **kw)
    np.testing.assert_array_equal(_raw(m.sample_device(y, n, S, **kw)), _raw(full))
    cuts = [0, n // 3 + 1, n - 333, n]
    parts = [m.sample_device(y, hi - lo, S, chain_offset=lo, **kw) for lo, hi in zip(cuts[:-1], cuts[1:])]
    np.testing.assert_array_equal(_raw(torch.cat(parts, 1)), _raw(full))
    for lo in (0, 35008, n - 1000):
        small = m.sample_device(y, 1000, S, chain_offset=lo, **kw)
        np.testing.assert_array_equal(_raw(small), _raw(full[:, lo:lo + 1000]))
    dmip._lib.device_status(torch.device(DEV))
    assert dmip._lib.calls["multistep_sample"] == before + 8
    assert torch.isfinite(full).all()
    assert not np.array_equal(_raw(full), _raw(m.sample_device(y, n, S, **dict(kw, seed=seed + 1))))


# ------------------------------------------------------------------------------ 4. trained weights
def _trained(dmip, tag):
    xd, yd, hl = {"lin": (2, 2, [64] * 3), "scat": (3, 23, [256] * 3)}[tag]
    m = dmip.CDE(xd, yd, hl)
    z = np.load(f"{GOLDEN}/ckpt_{tag}.npz")
    m.sde.a.load_state_dict(state_from_npz(z))
    return m, O.mlp_params_from_state(z)


@functools.lru_cache(maxsize=None)
def _trained_ref(tag, n, seed=1234):
    """(y, x0 of the samplers' own streams, f64 Heun-2048 reference) of a trained checkpoint, read-only."""
    params = O.mlp_params_from_state(np.load(f"{GOLDEN}/ckpt_{tag}.npz"))
    y = np.load(f"{GOLDEN}/flow_lmbd.npz")[f"{tag}_S10_y"]
    x0 = HR.x0_of_seed(seed, n, params[-1][0].shape[0])
    ref = HR.heun_sample(params, x0, y, 2048)
    ref.setflags(write=False)
    return y, x0, ref


@pytest.mark.parametrize("tag,n,prec", [("lin", 256, "fp32"), ("lin", 256, "fp32x3"), ("scat", 64, "fp32x3")])
def test_dpm2m_64_beats_heun_64_on_trained_weights(dmip, tag, n, prec):
    """Against the f64 Heun-2048 reference from the same x0: "dpm2m" at 64 evaluations errs less than the fused Heun
    sampler at 64 steps, which makes 128. The float64 prototype measured 6.6e-4 against 3.24e-3 on ckpt_lin and
    5.76e-3 against 9.94e-3 on ckpt_scat."""
    m, _ = _trained(dmip, tag)
    y, x0, ref = _trained_ref(tag, n)
    x0t = torch.from_numpy(x0)
    e_2m = HR.max_err(_sample(dmip, m, y, n, 64, "dpm2m", x0=x0t, precision=prec), ref)
    heun = m.sample_device(torch.from_numpy(np.asarray(y, np.float32)).to(DEV), n, 64, solver="heun", x0=x0t,
                           precision=prec)
    e_heun = HR.max_err(heun[0].cpu().numpy(), ref)
    print(f"{tag} {prec}: dpm2m-64 {e_2m:.3e}, Heun-64 (128 evaluations) {e_heun:.3e} (vs f64 Heun-2048)")
    assert e_2m < e_heun, (e_2m, e_heun)


# ------------------------------------------------------------------------------ 5. shared streams and x0=
@pytest.mark.parametrize("prec", ["fp32", "fp32x3"])
def test_same_x0_as_the_heun_sampler(dmip, prec):
    """One seed, internal RNG, ckpt_lin: "dpm2m" and Heun, both at S = 256, share the chains' streams (the same x0)
    and solve the same ODE, so they end within twice the sum of their own errors against Heun-2048, each measured on
    the CPU in f64 from that x0 (2M's is the 7e-4 of the final jump from t_end to 0); chains from another x0 would
    differ by the width of the posterior."""
    n, seed = 256, 1234
    m, params = _trained(dmip, "lin")
    y, x0, ref = _trained_ref("lin", n, seed)
    e_2m = HR.max_err(MR.table_sample(params, x0, y, MR.table_of(dmip, "dpm2m", "logsnr", 256)), ref)
    e_h = HR.max_err(HR.heun_sample(params, x0, y, 256), ref)
    a = _sample(dmip, m, y, n, 256, "dpm2m", seed=seed, precision=prec)
    b = m.sample_device(torch.from_numpy(y).to(DEV), n, 256, seed=seed, precision=prec, solver="heun")[0].cpu().numpy()
    d = HR.max_err(a, b)
    print(f"{prec}: |dpm2m-256 - Heun-256| = {d:.3e}; f64 errors {e_2m:.3e} (2M), {e_h:.3e} (Heun)")
    assert 0 < d <= 2 * (e_2m + e_h), (d, e_2m, e_h)
    assert HR.max_err(a, ref) <= 2 * e_2m


def test_x0_rows_follow_the_shard(dmip):
    """x0= with chain_offset holds the rows of the shard: a shard from x0[lo:hi] equals rows lo:hi of the full run
    (the chain's state does not depend on the RNG at all)."""
    torch.manual_seed(3)
    m = dmip.PosteriorDiffusionEstimator(2, 2, [64] * 3)
    ys = torch.randn(2, 2).to(DEV)
    n, S = 1000, 4
    x0 = torch.randn(2, n, 2)
    for prec in ("fp32", "fp32x3"):
        kw = dict(precision=prec, solver="dpm2m")
        full = m.sample_device(ys, n, S, seed=1, x0=x0, **kw)
        part = m.sample_device(ys, 301, S, seed=2, chain_offset=500, x0=x0[:, 500:801], **kw)
        np.testing.assert_array_equal(_raw(part), _raw(full[:, 500:801]))
        assert not torch.equal(full[0], full[1])
    # "fp16" runs the fp32x3 kernel: there is no 16-bit one
    np.testing.assert_array_equal(_raw(m.sample_device(ys, n, S, x0=x0, solver="dpm2m", precision="fp16")), _raw(full))


# ------------------------------------------------------------------------------ 6. snapshots
@pytest.mark.parametrize("prec", ["fp32", "fp32x3"])
@pytest.mark.parametrize("case", [HR.PARITY_CASES[0], HR.PARITY_CASES[3]], ids=lambda c: c[0])
def test_snapshots(dmip, case, prec):
    """snaps[-1] is the returned state bitwise (snapshot_every divides S); every snapshot is the restatement's state
    after that many steps, within bound 1 (internal RNG: the restatement starts from the stream's x0)."""
    kind, W, xd, yd, n = case
    m, params, prior, y, _, _ = _parity_ref(dmip, case, "dpm2m", "logsnr")
    S, every, seed = 6, 2, 99
    x0 = HR.x0_of_seed(seed, n, xd)
    _, ref_snaps = MR.direct_sample(params, x0, y, S, "dpm2m", "logsnr", prior, snapshot_every=every)
    before = dmip._lib.calls["multistep_sample"]
    yt = torch.from_numpy(y).to(DEV)
    x, snaps = m.sample_trajectory(yt, n, S, snapshot_every=every, seed=seed, precision=prec, solver="dpm2m")
    dmip._lib.device_status(torch.device(DEV))
    assert dmip._lib.calls["multistep_sample"] == before + 1
    assert snaps.shape == (3, 1, n, xd)
    np.testing.assert_array_equal(_raw(snaps[-1]), _raw(x))
    np.testing.assert_array_equal(_raw(x), _raw(m.sample_device(yt, n, S, seed=seed, precision=prec, solver="dpm2m")))
    for k in range(3):
        err = HR.max_err(snaps[k, 0].cpu().numpy(), ref_snaps[k])
        assert err < _bound(prec, ref_snaps[k]), (k, err)
    assert not torch.equal(snaps[0], snaps[-1])


# ------------------------------------------------------------------------------ 7. several ys in one launch
@pytest.mark.parametrize("prec", ["fp32", "fp32x3"])
def test_two_ys_in_one_launch(dmip, prec):
    """Two observations in one launch differ, and each equals its own single-y launch bitwise -- at a t_end and a grid
    other than the defaults too (the y index keys the chain's stream, so the single launch of ys[1] takes x0=)."""
    torch.manual_seed(11)
    m = dmip.CDE(3, 23, [128] * 2)
    ys = torch.randn(2, 23).to(DEV)
    n, S = 500, 5
    for kw in (dict(solver="dpm2m"), dict(solver="ddim", t_end=1e-2), dict(solver="dpm2m", grid="uniform")):
        x0 = torch.randn(2, n, 3, generator=torch.Generator().manual_seed(12))
        both = m.sample_device(ys, n, S, x0=x0, precision=prec, **kw)
        assert torch.isfinite(both).all() and not torch.equal(both[0], both[1])
        for k in range(2):
            one = m.sample_device(ys[k], n, S, x0=x0[k], precision=prec, **kw)
            np.testing.assert_array_equal(_raw(one[0]), _raw(both[k]))
    # internal RNG: y index 0 of a launch is the single-y launch of ys[0]
    both = m.sample_device(ys, n, S, seed=5, precision=prec, solver="dpm2m")
    np.testing.assert_array_equal(_raw(m.sample_device(ys[0], n, S, seed=5, precision=prec, solver="dpm2m")[0]),
                                  _raw(both[0]))
    assert not torch.equal(both[0], both[1])
    dmip._lib.device_status(torch.device(DEV))


def test_forward_takes_the_new_solvers(dmip):
    """model(y, ...) forwards solver=, grid= and t_end= through the sharded path: the chains of sample_device at the
    seed torch's generator hands out."""
    m, _ = _trained(dmip, "lin")
    m.sde.a.to(DEV)
    y = np.load(f"{GOLDEN}/flow_lmbd.npz")["lin_S10_y"].astype(np.float32)
    before = dmip._lib.calls["multistep_sample"]
    torch.manual_seed(21)
    a = m(torch.from_numpy(y).to(DEV), num_samples=300, num_steps=8, solver="dpm2m", t_end=1e-2)
    torch.manual_seed(21)
    seed = int(torch.randint(0, 2 ** 62, (1,)).item())
    b = m.sample_device(torch.from_numpy(y).to(DEV), 300, 8, seed=seed, solver="dpm2m", t_end=1e-2)[0].cpu().numpy()
    assert dmip._lib.calls["multistep_sample"] == before + 2
    assert isinstance(a, np.ndarray) and a.shape == (300, 2)
    np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))
