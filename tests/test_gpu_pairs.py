"""model.log_prob_pairs / model.sample_with_log_prob_pairs: the paired flow kernels, one observation per row
(csrc/dmip_flow_pairs.h, csrc/dmip_x3_flow_pairs.h; dmip_flow_logp_pairs, dmip_flow_sample_pairs), against the f64
restatements with a per-row y (tests/flow_ref.py, tests/flow_sample_ref.py: score_div broadcasts y to (n, ydim), so a
(n, ydim) y is taken row by row), against the per-y entry points and against themselves (single rows, slabs, shards),
and evaluate.hpd_coverage. Needs an MI355X: `pytest -m gpu`.

Gate of every accuracy test: flow_gpu.gate (tests/flow_cases.py), e_gpu <= 8 max(e_cpu, 1e-7) and never above the gate
it replaced, 4 e_cpu + 1e-6 (scaled by max(1, max |f64|) for the sampler's x and logq, as in test_gpu_flow_sample.py),
with e_cpu from the f32 restatement over the same rows. One f64 and one f32 run of each restatement per network, shared
read-only by the cases that slice them; rows are independent in the restatement too, so the first n rows of the
reference are the reference of the first n pairs.
"""
import importlib

import numpy as np
import pytest
import torch

import flow_cases as FC
import flow_ref as FR
import flow_sample_ref as FS
import heun_ref as HR
from flow_gpu import DEV, bits, case_model, dev, device_x0, gate, lin, post, seeded
from test_gpu_flow_logp import SHAPES

pytestmark = pytest.mark.gpu
PRECS = ["fp32", "fp32x3"]
SEED = 4242  # the samplers' seed


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


@pytest.fixture(scope="module")
def ev(dmip):
    return importlib.import_module(dmip.__name__ + ".evaluate")


_models, _logp_refs, _sample_refs = {}, {}, {}


def _ro(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def _case(dmip, golden, name):
    """(model, likelihood / CDE params, prior params or None, x (n, d), ys (n, ydim), S): the seeded CDE shapes of
    test_gpu_flow_logp.SHAPES (S = 6), a default-initialised Posterior pair at W 64 and the fixture pair at W 256, 21
    rows each. ys = default_rng(seed).normal(size=(n, ydim)): a different y in every row."""
    if name not in _models:
        if name in SHAPES:
            W, NL, xd, yd, n, S, seed = SHAPES[name]
            m, params = seeded(dmip, W, NL, xd, yd, seed)
            prior = None
        else:
            n, S, seed = 21, 6, 64 if name == "post64" else 256
            if name == "post64":
                torch.manual_seed(64)
                m = dmip.PosteriorDiffusionEstimator(2, 2, [64] * 3)
            else:
                m = post(dmip, golden)
            params, prior = HR.params_of(m.sde.a.likelihood_net), HR.params_of(m.sde.a.prior_net)
            xd, yd = m.xdim, m.ydim
        g = np.random.default_rng(seed)
        ys = g.normal(size=(n, yd)).astype(np.float32)
        x = g.normal(size=(n, xd)).astype(np.float32)
        _models[name] = (m, params, prior) + _ro(x, ys) + (S,)
    return _models[name]


def _logp_ref(dmip, golden, name):
    """(logp_f64, latent_f64, logp_f32, latent_f32) of the case's pairs, computed once."""
    if name not in _logp_refs:
        m, params, prior, x, ys, S = _case(dmip, golden, name)
        l64, z64 = FR.log_prob(params, x, ys, S, prior)
        l32, z32 = FR.log_prob(params, x, ys, S, prior, dtype=np.float32)
        _logp_refs[name] = _ro(l64, z64, l32, z32.astype(np.float64))
    return _logp_refs[name]


def _sample_ref(dmip, golden, name, S=None, offset=0):
    """(x0 from the device's generator at (SEED, offset + i, 0), ((x_f64, logq_f64), (x_f32, logq_f32)))."""
    key = (name, S, offset)
    if key not in _sample_refs:
        m, params, prior, x, ys, S0 = _case(dmip, golden, name)
        x0 = device_x0(dmip, SEED, offset, 0, len(ys), m.xdim)
        out = []
        for dtype in (np.float64, np.float32):
            xs, lq = FS.sample_with_logq(params, x0.cpu().numpy(), ys, S or S0, prior, dtype=dtype)
            out.append(_ro(xs, lq))
        _sample_refs[key] = (x0, out)
    return _sample_refs[key]


CASES = ["w64", "w128", "w512x1", "w512x3", "post64", "post256"]


# ------------------------------------------------------------------------------------- 1. accuracy, 3. launch count
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name", CASES)
def test_log_prob_pairs_vs_restatement(dmip, golden, name, prec):
    """logp and latent of every pair against the restatement with the rows' own y; one launch sequence per call."""
    m, _, _, x, ys, S = _case(dmip, golden, name)
    l64, z64, l32, z32 = _logp_ref(dmip, golden, name)
    before = dict(dmip._lib.calls)
    logp, lat = m.log_prob_pairs(dev(x), dev(ys), num_steps=S, return_latent=True, precision=prec)
    assert dmip._lib.calls["flow_logp_pairs"] == before.get("flow_logp_pairs", 0) + 1
    assert dmip._lib.calls.get("flow_logp", 0) == before.get("flow_logp", 0)
    assert logp.dtype == torch.float32 and logp.is_cuda and tuple(logp.shape) == (len(x),)
    assert tuple(lat.shape) == x.shape
    gate(f"{name} {prec} logp", logp.cpu().numpy(), l64, l32, scaled=False)
    gate(f"{name} {prec} latent", lat.cpu().numpy(), z64, z32, scaled=False)
    only = m.log_prob_pairs(dev(x), dev(ys), num_steps=S, precision=prec)
    np.testing.assert_array_equal(bits(only), bits(logp))


@pytest.mark.parametrize("scheme", FC.SCHEMES)
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("cid", list(FC.PAIRED))
def test_flow_cases_pairs_through_the_gate(dmip, golden, cid, prec, scheme):
    """The paired cases that tests/test_flow_accuracy_host.py proves the gate sharp on (a different y in every row; the
    seeded shapes and the fixture Posterior pair), both engines, both entry points, x0 injected: one launch each."""
    m = case_model(dmip, golden, cid)
    d = FC.data(cid)
    (run,) = d.runs
    r64, r32 = FC.refs(cid, scheme)
    call = "flow_logp_pairs" if scheme == "logp" else "flow_sample_pairs"
    before = dmip._lib.calls.get(call, 0)
    if scheme == "logp":
        logp, lat = m.log_prob_pairs(dev(run.x), dev(run.y), num_steps=d.S, return_latent=True, precision=prec)
        out = {"logp": logp, "latent": lat}
    else:
        x, logq = m.sample_with_log_prob_pairs(dev(run.y), d.S, x0=dev(run.x0), precision=prec)
        out = {"logq": logq, "x": x}
    assert dmip._lib.calls[call] == before + 1
    for arr in FC.ARRAYS[scheme]:
        gate(f"case {cid} {prec} {arr}", out[arr].cpu().numpy(), r64[arr], r32[arr], tag="FLOWGATE ")


# ------------------------------------------------------------------------------------- 2. ragged rows
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("n", [1, 3, 5, 17, 37])
def test_ragged_rows(dmip, golden, n, prec):
    """Row counts that are no multiple of the 4-row pass or of a workgroup's rows, W 64."""
    m, _, _, x, ys, S = _case(dmip, golden, "w64")
    l64, z64, l32, z32 = _logp_ref(dmip, golden, "w64")
    logp, lat = m.log_prob_pairs(dev(x[:n]), dev(ys[:n]), num_steps=S, return_latent=True, precision=prec)
    assert tuple(logp.shape) == (n,) and tuple(lat.shape) == (n, 2)
    gate(f"w64 n={n} {prec} logp", logp.cpu().numpy(), l64[:n], l32[:n], scaled=False)
    gate(f"w64 n={n} {prec} latent", lat.cpu().numpy(), z64[:n], z32[:n], scaled=False)


# ------------------------------------------------------------------------------------- 4. its own y per row
@pytest.mark.parametrize("prec", PRECS)
def test_every_row_reads_its_own_y(dmip, golden, prec):
    """Permuting the rows of y moves logp by more than 1e-3; rows that share one y agree with log_prob(x, y0) within
    the gate (bit for bit or not is printed: DESIGN.md 3i records it, nothing asserts it)."""
    m, params, _, x, ys, S = _case(dmip, golden, "w64")
    logp = m.log_prob_pairs(dev(x), dev(ys), num_steps=S, precision=prec).cpu().numpy()
    rolled = m.log_prob_pairs(dev(x), dev(np.roll(ys, 1, axis=0)), num_steps=S, precision=prec).cpu().numpy()
    assert np.abs(rolled - logp).max() > 1e-3
    y0 = np.repeat(ys[:1], len(x), axis=0)
    shared = m.log_prob_pairs(dev(x), dev(y0), num_steps=S, precision=prec)
    per_y = m.log_prob(dev(x), dev(ys[0]), num_steps=S, precision=prec)
    l64, _ = FR.log_prob(params, x, ys[0], S)
    l32, _ = FR.log_prob(params, x, ys[0], S, dtype=np.float32)
    gate(f"shared y {prec} pairs", shared.cpu().numpy(), l64, l32, scaled=False)
    gate(f"shared y {prec} per-y", per_y.cpu().numpy(), l64, l32, scaled=False)
    same = int((bits(shared) == bits(per_y)).sum())
    print(f"shared y, {prec}: {same} of {len(x)} rows bitwise equal to log_prob(x, y0); max |diff| "
          f"{(shared - per_y).abs().max().item():.3e}")


# ------------------------------------------------------------------------------------- 5. row independence, slabs
@pytest.mark.parametrize("prec", PRECS)
def test_row_independence_and_slabs_bitwise(dmip, golden, prec, monkeypatch):
    """Row r alone is bitwise row r among 37 (r = 0, 3, 4, 16, 36), and a run forced into slabs of 5 rows (the host
    layer's test hook DMIP_PAIRS_SLAB_ROWS) is bitwise the unslabbed run, for log_prob_pairs and for the sampler."""
    m, _, _, x, ys, S = _case(dmip, golden, "w64")
    monkeypatch.delenv("DMIP_PAIRS_SLAB_ROWS", raising=False)
    full, lat = m.log_prob_pairs(dev(x), dev(ys), num_steps=S, return_latent=True, precision=prec)
    xs, lq = m.sample_with_log_prob_pairs(dev(ys), S, seed=SEED, precision=prec)
    for r in (0, 3, 4, 16, 36):
        one, lat1 = m.log_prob_pairs(dev(x[r:r + 1]), dev(ys[r:r + 1]), num_steps=S, return_latent=True,
                                     precision=prec)
        np.testing.assert_array_equal(bits(one), bits(full[r:r + 1]))
        np.testing.assert_array_equal(bits(lat1), bits(lat[r:r + 1]))
    monkeypatch.setenv("DMIP_PAIRS_SLAB_ROWS", "5")
    slab, slat = m.log_prob_pairs(dev(x), dev(ys), num_steps=S, return_latent=True, precision=prec)
    sxs, slq = m.sample_with_log_prob_pairs(dev(ys), S, seed=SEED, precision=prec)
    np.testing.assert_array_equal(bits(slab), bits(full))
    np.testing.assert_array_equal(bits(slat), bits(lat))
    np.testing.assert_array_equal(bits(sxs), bits(xs))
    np.testing.assert_array_equal(bits(slq), bits(lq))


# ------------------------------------------------------------------------------------- 6. paired sampling
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name", CASES)
def test_sample_pairs_vs_restatement(dmip, golden, name, prec):
    """x and logq from the device's own start states (flow_gpu.device_x0 at (SEED, i, 0)) against sample_with_logq
    with per-row y; the seeded path gives the bits of the x0= path handed those start states."""
    m, _, _, _, ys, S = _case(dmip, golden, name)
    x0, ((x64, l64), (x32, l32)) = _sample_ref(dmip, golden, name)
    before = dmip._lib.calls.get("flow_sample_pairs", 0)
    x, logq = m.sample_with_log_prob_pairs(dev(ys), S, seed=SEED, precision=prec)
    assert dmip._lib.calls["flow_sample_pairs"] == before + 1
    assert tuple(x.shape) == (len(ys), m.xdim) and tuple(logq.shape) == (len(ys),)
    assert x.dtype == logq.dtype == torch.float32 and x.is_cuda and logq.is_cuda
    gate(f"{name} {prec} logq", logq.cpu().numpy(), l64, l32)
    gate(f"{name} {prec} x", x.cpu().numpy(), x64, x32)
    xi, lqi = m.sample_with_log_prob_pairs(dev(ys), S, seed=SEED + 1, x0=x0.clone(), precision=prec)
    np.testing.assert_array_equal(bits(xi), bits(x))
    np.testing.assert_array_equal(bits(lqi), bits(logq))


@pytest.mark.parametrize("prec", PRECS)
def test_sample_pairs_shards_are_the_whole_run(dmip, golden, prec):
    """Two chain_offset shards (rows sliced at 13, no multiple of a pass) equal the whole run's bits."""
    m, _, _, _, ys, S = _case(dmip, golden, "w64")
    x, logq = m.sample_with_log_prob_pairs(dev(ys), S, seed=SEED, chain_offset=100, precision=prec)
    xa, la = m.sample_with_log_prob_pairs(dev(ys[:13]), S, seed=SEED, chain_offset=100, precision=prec)
    xb, lb = m.sample_with_log_prob_pairs(dev(ys[13:]), S, seed=SEED, chain_offset=113, precision=prec)
    np.testing.assert_array_equal(bits(torch.cat([xa, xb])), bits(x))
    np.testing.assert_array_equal(bits(torch.cat([la, lb])), bits(logq))


@pytest.mark.parametrize("prec", PRECS)
def test_sample_pairs_start_is_the_per_y_sampler_start(dmip, golden, prec):
    """Row i starts where sample_with_log_prob(ys[i], 1, seed, chain_offset=i) starts: at S = 1 the outputs of the two
    agree within the gate (five rows), and both pass it against the restatement from the device's start states."""
    m, _, _, _, ys, _ = _case(dmip, golden, "w64")
    x0, ((x64, l64), (x32, l32)) = _sample_ref(dmip, golden, "w64", S=1)
    x, logq = m.sample_with_log_prob_pairs(dev(ys), 1, seed=SEED, precision=prec)
    gate(f"S=1 {prec} pairs x", x.cpu().numpy(), x64, x32)
    for i in (0, 3, 4, 16, 36):
        xi, lqi = m.sample_with_log_prob(dev(ys[i]), 1, 1, seed=SEED, chain_offset=i, precision=prec)
        gate(f"S=1 {prec} row {i} per-y x", xi.cpu().numpy(), x64[i:i + 1], x32[i:i + 1])
        gate(f"S=1 {prec} row {i} per-y logq", lqi.cpu().numpy(), l64[i:i + 1], l32[i:i + 1])
        gate(f"S=1 {prec} row {i} pairs x", x[i:i + 1].cpu().numpy(), x64[i:i + 1], x32[i:i + 1])
        gate(f"S=1 {prec} row {i} pairs logq", logq[i:i + 1].cpu().numpy(), l64[i:i + 1], l32[i:i + 1])


# ------------------------------------------------------------------------------------- 7. encode / decode
@pytest.mark.parametrize("prec", PRECS)
def test_encode_decode_round_trip(dmip, golden, prec):
    """x -> latent (log_prob_pairs) -> x (sample_with_log_prob_pairs, x0 = latent) at S = 64 on ckpt_lin, 16 pairs:
    within twice the same round trip's error in the f64 restatement, plus 1e-4 (the tolerance of
    test_gpu_heun.test_round_trip_through_log_prob)."""
    m = lin(dmip, golden)
    params = HR.params_of(m.sde.a)
    g = np.random.default_rng(6)
    x = g.normal(size=(16, 2)).astype(np.float32)
    ys = g.normal(size=(16, 2)).astype(np.float32)
    _, lat_ref = FR.log_prob(params, x, ys, 64)
    back_ref, _ = FS.sample_with_logq(params, lat_ref.astype(np.float32), ys, 64)
    e_ref = np.abs(back_ref - x).max()
    logp, lat = m.log_prob_pairs(dev(x), dev(ys), num_steps=64, return_latent=True, precision=prec)
    back, logq = m.sample_with_log_prob_pairs(dev(ys), 64, x0=lat, precision=prec)
    e = np.abs(back.cpu().numpy() - x).max()
    print(f"{prec} round trip |x_back - x|: device {e:.3e}, f64 restatement {e_ref:.3e}")
    assert torch.isfinite(logp).all() and torch.isfinite(logq).all() and e <= 2 * e_ref + 1e-4, (e, e_ref)


# ------------------------------------------------------------------------------------- 8. range
def test_a_row_beyond_the_split_range_raises(dmip, golden):
    """One row at |x| = 1e5 > 65504 among nine: precision="fp32x3" raises "fp16 range"; exact f32 does not."""
    m = lin(dmip, golden)
    g = np.random.default_rng(8)
    x = g.normal(size=(9, 2)).astype(np.float32)
    ys = g.normal(size=(9, 2)).astype(np.float32)
    x[4] = (1e5, -1e5)
    with pytest.raises(RuntimeError, match="fp16 range"):
        m.log_prob_pairs(dev(x), dev(ys), num_steps=4, precision="fp32x3")
    logp = m.log_prob_pairs(dev(x), dev(ys), num_steps=4, precision="fp32").cpu().numpy()
    assert not np.any(np.isnan(logp)) and np.all(np.isfinite(np.delete(logp, 4)))
    ok = m.log_prob_pairs(dev(np.delete(x, 4, axis=0)), dev(np.delete(ys, 4, axis=0)), num_steps=4, precision="fp32x3")
    assert torch.isfinite(ok).all()  # the status word is clear again
    with pytest.raises(RuntimeError, match="fp16 range"):
        m.sample_with_log_prob_pairs(dev(ys), 4, x0=dev(x), precision="fp32x3")
    xs, lq = m.sample_with_log_prob_pairs(dev(ys), 4, x0=dev(x), precision="fp32")
    assert not torch.isnan(lq).any()


# ------------------------------------------------------------------------------------- 9. hpd_coverage
@pytest.mark.parametrize("prec", PRECS)
def test_hpd_coverage_counts(dmip, golden, ev, prec):
    """ckpt_lin, 64 pairs of LinearForwardProblem's joint (x ~ N(0, I), y = A x + b + N(0, 0.3 I)), L = 64, S = 20:
    alpha_i of five pairs equals the count recomputed from per-y calls at the same seed --
    sample_with_log_prob(y_i, L, x0 = the start states of y index i's streams) and log_prob(x_true_i, y_i). The two
    routes' logq agree only within the gate, so the five are the first pairs whose truth is further from every
    sample's logq than twice the gate's width (4 e_cpu + 1e-6, e_cpu of the truths' f32 restatement; one width for
    each side of the comparison). No statistical claim on the trained model."""
    m = lin(dmip, golden)
    params = HR.params_of(m.sde.a)
    n, L, S = 64, 64, 20
    prob = dmip.LinearForwardProblem()
    g = torch.Generator().manual_seed(9)
    x_true = torch.randn(n, 2, generator=g)
    y = prob.forward(x_true) + prob.scale ** 0.5 * torch.randn(n, 2, generator=g)
    before = dict(dmip._lib.calls)
    rep = ev.hpd_coverage(m, x_true.to(DEV), y.to(DEV), L, num_steps=S, seed=SEED, precision=prec)
    assert dmip._lib.calls["flow_logp_pairs"] == before.get("flow_logp_pairs", 0) + 1
    assert dmip._lib.calls["flow_sample"] == before.get("flow_sample", 0) + 1
    lt, ls = rep["logq_truth"].cpu().numpy().astype(np.float64), rep["logq_samples"].cpu().numpy().astype(np.float64)
    assert lt.shape == (n,) and ls.shape == (n, L) and rep["alpha"].shape == (n,)
    assert np.array_equal(rep["alpha"], (ls > lt[:, None]).sum(1) / L)
    assert np.array_equal(rep["coverage"], (rep["alpha"][:, None] <= rep["levels"][None, :]).mean(0))
    l64, _ = FR.log_prob(params, x_true.numpy(), y.numpy(), S)
    l32, _ = FR.log_prob(params, x_true.numpy(), y.numpy(), S, dtype=np.float32)
    width = 4 * np.abs(l32 - l64).max() + 1e-6
    clear = [i for i in range(n) if np.abs(ls[i] - lt[i]).min() > 2 * width][:5]
    assert len(clear) == 5, (clear, width)
    for i in clear:
        x0 = device_x0(dmip, SEED, 0, i, L, 2)  # the multi-y call drew y index i's chains from stream i
        _, lq = m.sample_with_log_prob(y[i].to(DEV), L, S, x0=x0, precision=prec)
        lp = m.log_prob(x_true[i:i + 1].to(DEV), y[i].to(DEV), num_steps=S, precision=prec)
        assert abs(float(lp[0]) - lt[i]) <= width and np.abs(lq.cpu().numpy() - ls[i]).max() <= width
        count = int((lq.double() > lp.double()).sum())
        assert count / L == rep["alpha"][i], (i, count, rep["alpha"][i])


# ------------------------------------------------------------------------------------- refusals
def test_refusals_launch_nothing(dmip):
    """A width without a kernel, a SiLU network, CDiffE, mismatched rows and std = 0 raise ValueError before any
    launch; so does the C-ABI for a SiLU handle and for a prior and a likelihood of different hidden layers."""
    x, y = torch.zeros(4, 3, device=DEV), torch.zeros(4, 23, device=DEV)
    m = dmip.CDE(3, 23, [256] * 3)
    silu = dmip.CDE(3, 23, [256] * 3)
    silu.sde.a = dmip.MLP(3 + 23 + 1, 3, [256] * 3, torch.nn.SiLU()).to(DEV)
    before = dict(dmip._lib.calls)
    for bad in (dmip.CDE(3, 23, [96] * 3), silu):
        with pytest.raises(ValueError):
            bad.log_prob_pairs(x, y, num_steps=4)
        with pytest.raises(ValueError):
            bad.sample_with_log_prob_pairs(y, 4)
    with pytest.raises(ValueError, match="log_prob_pairs"):
        dmip.CDiffE(3, 23, [256] * 3).log_prob_pairs(x, y)
    with pytest.raises(ValueError, match="rows"):
        m.log_prob_pairs(x, y[:3], num_steps=4)
    with pytest.raises(ValueError, match="std"):
        m.sample_with_log_prob_pairs(y, 4, std=0)
    with pytest.raises(ValueError, match="x0"):
        m.sample_with_log_prob_pairs(y, 4, x0=torch.zeros(3, 3))
    assert dict(dmip._lib.calls) == before
    L = dmip._lib
    logp = torch.empty(4, device=DEV)
    with pytest.raises(ValueError, match="tanh"):
        L.flow_logp_pairs(L.DMIP_SAMPLER_CDE, silu.sde.a.dmip_handle(torch.device(DEV), 3), None,
                          L.vpsde(0.1, 20.0, 1.0), x, y, 4, logp)
    # a prior and a likelihood of different hidden layers
    pa, pb = dmip.PosteriorDiffusionEstimator(2, 2, [64] * 3), dmip.PosteriorDiffusionEstimator(2, 2, [128] * 3)
    lik = pa.sde.a.likelihood_net.dmip_handle(torch.device(DEV), 2)
    pri = pb.sde.a.prior_net.dmip_handle(torch.device(DEV), 2)
    x2, y2, xo = torch.zeros(4, 2, device=DEV), torch.zeros(4, 2, device=DEV), torch.empty(4, 2, device=DEV)
    with pytest.raises(ValueError, match="same hidden layers"):
        L.flow_logp_pairs(L.DMIP_SAMPLER_POSTERIOR, lik, pri, L.vpsde(0.1, 20.0, 1.0), x2, y2, 4, logp)
    with pytest.raises(ValueError, match="same hidden layers"):
        L.flow_sample_pairs(L.DMIP_SAMPLER_POSTERIOR, lik, pri, L.vpsde(0.1, 20.0, 1.0), y2, 0, 4, 0.0, 1.0, 1, xo, logp)
    with pytest.raises(ValueError, match="tanh"):
        L.flow_sample_pairs(L.DMIP_SAMPLER_CDE, silu.sde.a.dmip_handle(torch.device(DEV), 3), None,
                            L.vpsde(0.1, 20.0, 1.0), y, 0, 4, 0.0, 1.0, 1, torch.empty(4, 3, device=DEV), logp)
    torch.cuda.synchronize()
