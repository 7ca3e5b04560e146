"""model.log_prob and model.sample_with_log_prob at precision="fp32x3": the flow kernels on the split-fp16 engine
(csrc/dmip_x3_flow.h, dmip_flow_logp_ex / dmip_flow_sample_ex) against the f64 restatements (tests/flow_ref.py,
tests/flow_sample_ref.py), the fp32x3 Heun sampler, themselves (shards, single rows, seed path / x0 path), the
exact-f32 kernels and evaluate.importance_posterior. Needs an MI355X: `pytest -m gpu`.

Gate of every accuracy test (flow_cases.gate, every flow test's): with e_gpu = max |gpu - f64| and e_cpu = max |f32
restatement - f64| over the same rows -- the restatement's own f32 run, never the code under test --
    e_gpu <= K max(e_cpu, 1e-7),   K = 8
and never above the gate it replaced, 4 e_cpu + 1e-6 max(1, max |f64|). tests/flow_cases.py derives K and
tests/test_flow_accuracy_host.py proves on the CPU that a tangent path with a lost product or flushed lo halves misses
it; measured e_gpu / max(e_cpu, 1e-7) on the device: DESIGN.md 3g. One f64 and one f32 run of a restatement per
network and y, shared read-only by the cases that slice them.
"""
import functools
import importlib

import numpy as np
import pytest
import torch

import flow_cases as FC
import flow_ref as FR
import flow_sample_ref as FS
import heun_ref as HR
from flow_gpu import DEV, case_model, gate, seeded
from flow_gpu import bits as _bits, dev as _dev, device_x0 as _device_x0, sample_reference as _sample_reference
from flow_gpu import lin as _lin, post as _post, scat as _scat

pytestmark = pytest.mark.gpu

X3 = "fp32x3"


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


@pytest.fixture(scope="module")
def ev(dmip):
    return importlib.import_module(dmip.__name__ + ".evaluate")


def _gate(name, got, ref64, ref32):
    gate(name, got, ref64, ref32, tag="X3GATE ")


# ------------------------------------------------------------------------------------- 1. fixture checkpoints
@pytest.mark.parametrize("case", ["a", "b", "d"])
def test_log_prob_fixture_cases(dmip, golden, case):
    """flow_logp.npz (a) ckpt_lin 37 rows S = 20, (b) ckpt_scat 50 rows S = 10, (d) the Posterior pair, 21 rows x 2
    ys, S = 6: one flow_logp call each, against the fixture's f64 values (its own f32 run is e_cpu)."""
    z = golden("flow_logp.npz")
    m = {"a": _lin, "b": _scat, "d": _post}[case](dmip, golden)
    before = dmip._lib.calls.get("flow_logp", 0)
    logp, lat = m.log_prob(_dev(z[f"{case}_x"]), _dev(z[f"{case}_y"]), num_steps=int(z[f"{case}_S"]),
                           return_latent=True, precision=X3)
    assert dmip._lib.calls["flow_logp"] == before + 1
    assert logp.dtype == torch.float32 and logp.is_cuda
    assert tuple(logp.shape) == z[f"{case}_logp_f64"].shape and tuple(lat.shape) == z[f"{case}_x"].shape
    _gate(f"logp ({case}) logp", logp.cpu().numpy(), z[f"{case}_logp_f64"], z[f"{case}_logp_f32_cpu"])
    _gate(f"logp ({case}) latent", lat.cpu().numpy(), z[f"{case}_latent_f64"], z[f"{case}_latent_f32_cpu"])


@pytest.mark.parametrize("case", ["lin", "scat", "post"])
def test_sample_fixture_cases(dmip, golden, case):
    """The same checkpoints, ys, row counts and step counts through sample_with_log_prob, x0 injected (the device's
    Box-Muller normals are only within 2e-5 of the oracle's): one flow_sample call each."""
    z = golden("flow_logp.npz")
    if case == "lin":
        m, ys, n, S, prior = _lin(dmip, golden), z["a_y"][None], 37, 20, None
        params = HR.params_of(m.sde.a)
    elif case == "scat":
        m, ys, n, S, prior = _scat(dmip, golden), z["b_y"][None], 50, 10, None
        params = HR.params_of(m.sde.a)
    else:
        m, ys, n, S = _post(dmip, golden), z["d_y"], 21, 6
        params, prior = HR.params_of(m.sde.a.likelihood_net), HR.params_of(m.sde.a.prior_net)
    x0 = np.stack([HR.x0_of_seed(1234, n, m.xdim, stream=i) for i in range(len(ys))])
    before = dmip._lib.calls.get("flow_sample", 0)
    if len(ys) == 1:
        x, logq = m.sample_with_log_prob(_dev(ys[0]), n, S, x0=_dev(x0[0]), precision=X3)
        assert tuple(x.shape) == (n, m.xdim) and tuple(logq.shape) == (n,)
        x, logq = x[None], logq[None]
    else:
        x, logq = m.sample_with_log_prob(_dev(ys), n, S, x0=_dev(x0), precision=X3)
        assert tuple(x.shape) == (len(ys), n, m.xdim) and tuple(logq.shape) == (len(ys), n)
    assert dmip._lib.calls["flow_sample"] == before + 1
    assert x.dtype == logq.dtype == torch.float32 and x.is_cuda and logq.is_cuda
    for i in range(len(ys)):
        (x64, l64), (x32, l32) = _sample_reference(params, x0[i], ys[i], S, prior)
        _gate(f"sample ({case}, y {i}) logq", logq[i].cpu().numpy(), l64, l32)
        _gate(f"sample ({case}, y {i}) x", x[i].cpu().numpy(), x64, x32)


# ------------------------------------------------------------------------------------- 1. seeded networks
SHAPES = FC.SHAPES  # name: (W, n_hidden, xdim, ydim, rows of the shared reference, weight seed); S = 4
S_SEEDED = FC.S_SEEDED
_refs = {}


def _seeded(dmip, name):
    """(model, rows x (n, d) -- of log_prob, and the x0 of sample_with_log_prob --, ys (3, ydim), per-y references
    {"logp": (l64, z64, l32, z32), "sample": ((x64, q64), (x32, q32))}) -- computed once per shape, shared,
    unchanged."""
    W, NL, xd, yd, n, seed = SHAPES[name]
    m, params = seeded(dmip, W, NL, xd, yd, seed)
    if name not in _refs:
        ys = np.random.default_rng(seed).normal(size=(3, yd)).astype(np.float32)
        n_y = 3 if name == "w64" else 1
        x = HR.x0_of_seed(seed, n, xd)
        x.setflags(write=False)
        ref = []
        for i in range(n_y):
            l64, z64 = FR.log_prob(params, x, ys[i], S_SEEDED)
            l32, z32 = FR.log_prob(params, x, ys[i], S_SEEDED, dtype=np.float32)
            for a in (l64, z64, l32, z32):
                a.setflags(write=False)
            ref.append({"logp": (l64, z64, l32, z32), "sample": _sample_reference(params, x, ys[i], S_SEEDED)})
        _refs[name] = (x, ys, ref)
    x, ys, ref = _refs[name]
    return m, x, ys, ref


@pytest.mark.parametrize("name,n", [("w64", 1), ("w64", 3), ("w64", 5), ("w64", 17), ("w64", 37), ("w128", 19),
                                    ("w64x1", 21), ("w512", 21)])
def test_seeded_networks_and_ragged_rows(dmip, name, n):
    """W 64 and 128 with 3 hidden layers, W 64 with one (no streamed hidden tile), W 512 with ydim 23 (compiled: it is
    free of scratch); S = 4; for W 64 row counts that are no multiple of the 4-row pass. Both entry points."""
    m, x, ys, ref = _seeded(dmip, name)
    l64, z64, l32, z32 = ref[0]["logp"]
    logp, lat = m.log_prob(_dev(x[:n]), _dev(ys[0]), num_steps=S_SEEDED, return_latent=True, precision=X3)
    assert tuple(logp.shape) == (n,) and tuple(lat.shape) == (n, x.shape[1])
    _gate(f"logp {name} n={n} logp", logp.cpu().numpy(), l64[:n], l32[:n])
    _gate(f"logp {name} n={n} latent", lat.cpu().numpy(), z64[:n], z32[:n])
    (x64, q64), (x32, q32) = ref[0]["sample"]
    xs, logq = m.sample_with_log_prob(_dev(ys[0]), n, S_SEEDED, x0=_dev(x[:n]), precision=X3)
    assert tuple(xs.shape) == (n, x.shape[1]) and tuple(logq.shape) == (n,)
    _gate(f"sample {name} n={n} logq", logq.cpu().numpy(), q64[:n], q32[:n])
    _gate(f"sample {name} n={n} x", xs.cpu().numpy(), x64[:n], x32[:n])


def test_multi_y(dmip):
    """n_y = 3, a different y each: every y index reads its own layer-1 bias and its own rows."""
    m, x, ys, ref = _seeded(dmip, "w64")
    n = 5
    rows = np.stack([x[:n]] * 3)
    logp = m.log_prob(_dev(rows), _dev(ys), num_steps=S_SEEDED, precision=X3)
    xs, logq = m.sample_with_log_prob(_dev(ys), n, S_SEEDED, x0=_dev(rows), precision=X3)
    assert tuple(logp.shape) == (3, n) and tuple(xs.shape) == (3, n, 2) and tuple(logq.shape) == (3, n)
    for i in range(3):
        l64, _, l32, _ = ref[i]["logp"]
        (x64, q64), (x32, q32) = ref[i]["sample"]
        _gate(f"multi-y {i} logp", logp[i].cpu().numpy(), l64[:n], l32[:n])
        _gate(f"multi-y {i} logq", logq[i].cpu().numpy(), q64[:n], q32[:n])
        _gate(f"multi-y {i} x", xs[i].cpu().numpy(), x64[:n], x32[:n])
    assert np.abs(logp[0].cpu().numpy() - ref[1]["logp"][0][:n]).max() > 1e-3  # the ys do differ


# ------------------------------------------------------------------------------------- 1. the cases of flow_cases
@pytest.mark.parametrize("scheme", FC.SCHEMES)
@pytest.mark.parametrize("prec", [X3, "fp32"])
@pytest.mark.parametrize("cid", [c for c in FC.CASES if c not in FC.PAIRED])
def test_flow_cases_through_the_gate(dmip, golden, cid, prec, scheme):
    """Every case that tests/test_flow_accuracy_host.py proves the gate sharp on, on both engines and both entry
    points, x0 injected: one launch each (case d: its two ys in one), against flow_cases' own restatements."""
    m = case_model(dmip, golden, cid)
    d = FC.data(cid)
    r64, r32 = FC.refs(cid, scheme)
    one = len(d.runs) == 1
    pick = (lambda a: _dev(a[0])) if one else _dev
    ys = pick(np.stack([r.y for r in d.runs]))
    call = "flow_logp" if scheme == "logp" else "flow_sample"
    before = dmip._lib.calls.get(call, 0)
    if scheme == "logp":
        logp, lat = m.log_prob(pick(np.stack([r.x for r in d.runs])), ys, num_steps=d.S, return_latent=True,
                               precision=prec)
        out = {"logp": logp, "latent": lat}
    else:
        x, logq = m.sample_with_log_prob(ys, len(d.runs[0].x0), d.S, x0=pick(np.stack([r.x0 for r in d.runs])),
                                         precision=prec)
        out = {"logq": logq, "x": x}
    assert dmip._lib.calls[call] == before + 1
    for arr in FC.ARRAYS[scheme]:
        got = out[arr].cpu().numpy().reshape(r64[arr].shape)
        gate(f"case {cid} {prec} {arr}", got, r64[arr], r32[arr], tag="FLOWGATE ")


# ------------------------------------------------------------------------------------- 2. the fp32x3 Heun sampler
@pytest.mark.parametrize("case", ["lin", "scat"])
def test_same_x_as_the_fp32x3_heun_sampler(dmip, golden, case):
    """Seed path against sample_device(solver="heun", precision="fp32x3") at the same seed, 100 rows, S = 8: the
    same HeunStep, engine, images and RNG, and an MFMA column does not depend on its neighbours (16 primal columns
    there, 4 primal + 12 tangent columns here). Bitwise equality."""
    m = _lin(dmip, golden) if case == "lin" else _scat(dmip, golden)
    y = _dev(golden("flow_logp.npz")["a_y" if case == "lin" else "b_y"])
    pairs = []
    for seed in (7, 2 ** 40 + 3):
        ref = m.sample_device(y, 100, 8, seed=seed, precision=X3, solver="heun")[0]
        x, _ = m.sample_with_log_prob(y, 100, 8, seed=seed, precision=X3)
        d = (x - ref).abs().max().item()
        same = bool(np.array_equal(_bits(x), _bits(ref)))
        print(f"X3HEUN ({case}, seed {seed}) max |x - x_heun| = {d:.3e}, bitwise {same}, max |ref| = "
              f"{ref.abs().max().item():.4g}")
        assert torch.isfinite(x).all()
        pairs.append((x, ref))
    for x, ref in pairs:
        np.testing.assert_array_equal(_bits(x), _bits(ref))


# ------------------------------------------------------------------------------------- 3. bitwise invariances
def test_shards_and_single_rows_are_bitwise_the_whole_run(dmip, golden):
    """Rows 500..800 alone (chain_offset = 500, 301 rows) equal those rows of a 1,000-row run; one row alone equals
    the same row among 37, for both entry points (quad / column cross-talk in the DPP broadcast or the output
    shuffles would show here)."""
    m = _lin(dmip, golden)
    y = _dev(golden("flow_logp.npz")["a_y"])
    S, seed = 4, 31
    x, logq = m.sample_with_log_prob(y, 1000, S, seed=seed, precision=X3)
    xs, ls = m.sample_with_log_prob(y, 301, S, seed=seed, chain_offset=500, precision=X3)
    np.testing.assert_array_equal(_bits(xs), _bits(x[500:801]))
    np.testing.assert_array_equal(_bits(ls), _bits(logq[500:801]))
    x37, l37 = m.sample_with_log_prob(y, 37, S, seed=seed, precision=X3)
    np.testing.assert_array_equal(_bits(x37), _bits(x[:37]))
    rows = x[:37].contiguous()
    p37, z37 = m.log_prob(rows, y, num_steps=S, return_latent=True, precision=X3)
    # rows 500..800 of log_prob: a slice of the rows is a run of its own
    pa = m.log_prob(x, y, num_steps=S, precision=X3)
    pb = m.log_prob(x[500:801].contiguous(), y, num_steps=S, precision=X3)
    np.testing.assert_array_equal(_bits(pb), _bits(pa[500:801]))
    np.testing.assert_array_equal(_bits(p37), _bits(pa[:37]))
    for r in (0, 3, 4, 16, 36):
        x1, l1 = m.sample_with_log_prob(y, 1, S, seed=seed, chain_offset=r, precision=X3)
        np.testing.assert_array_equal(_bits(x1), _bits(x37[r:r + 1]))
        np.testing.assert_array_equal(_bits(l1), _bits(l37[r:r + 1]))
        p1, z1 = m.log_prob(rows[r:r + 1], y, num_steps=S, return_latent=True, precision=X3)
        np.testing.assert_array_equal(_bits(p1), _bits(p37[r:r + 1]))
        np.testing.assert_array_equal(_bits(z1), _bits(z37[r:r + 1]))


@pytest.mark.parametrize("case,mean,std", [("lin", 0.0, 1.0), ("lin", 0.3, 1.5), ("scat", 0.0, 1.0)])
def test_seed_path_equals_x0_path(dmip, golden, case, mean, std):
    """The chains' own start states (dmip_rng_normals, times std plus mean) passed back as x0= give (x, logq) bit for
    bit; n_y = 2 (each y its own stream), and mean = 0.3, std = 1.5 (the base density's -d log std and residual)."""
    m = _lin(dmip, golden) if case == "lin" else _scat(dmip, golden)
    y = golden("flow_logp.npz")["a_y" if case == "lin" else "b_y"]
    ys = _dev(np.stack([y, 0.5 * y]))
    n, S, seed = 45, 5, 99
    x, logq = m.sample_with_log_prob(ys, n, S, mean=mean, std=std, seed=seed, chain_offset=11, precision=X3)
    x0 = torch.stack([_device_x0(dmip, seed, 11, i, n, m.xdim, mean, std) for i in range(2)])
    x2, logq2 = m.sample_with_log_prob(ys, n, S, mean=mean, std=std, seed=seed + 1, x0=x0, precision=X3)
    assert torch.isfinite(logq).all() and (x[0] - x[1]).abs().max().item() > 1e-3
    np.testing.assert_array_equal(_bits(x2), _bits(x))
    np.testing.assert_array_equal(_bits(logq2), _bits(logq))


# ------------------------------------------------------------------------------------- 4. the default is unchanged
def test_default_precision_is_exact_f32(dmip, golden):
    """No `precision` is precision="fp32", bit for bit, for both entry points -- and not the split engine's bits."""
    m = _scat(dmip, golden)
    z = golden("flow_logp.npz")
    x, y = _dev(z["b_x"]), _dev(z["b_y"])
    a = m.log_prob(x, y, num_steps=6)
    b = m.log_prob(x, y, num_steps=6, precision="fp32")
    c = m.log_prob(x, y, num_steps=6, precision=X3)
    np.testing.assert_array_equal(_bits(a), _bits(b))
    assert not np.array_equal(_bits(a), _bits(c))
    xa, qa = m.sample_with_log_prob(y, 50, 6, seed=5)
    xb, qb = m.sample_with_log_prob(y, 50, 6, seed=5, precision="fp32")
    xc, qc = m.sample_with_log_prob(y, 50, 6, seed=5, precision=X3)
    np.testing.assert_array_equal(_bits(xa), _bits(xb))
    np.testing.assert_array_equal(_bits(qa), _bits(qb))
    assert not np.array_equal(_bits(qa), _bits(qc))
    # "fp16" and "bf16" run the split engine
    for prec in ("fp16", "bf16"):
        xd, qd = m.sample_with_log_prob(y, 50, 6, seed=5, precision=prec)
        np.testing.assert_array_equal(_bits(xd), _bits(xc))
        np.testing.assert_array_equal(_bits(qd), _bits(qc))
        np.testing.assert_array_equal(_bits(m.log_prob(x, y, num_steps=6, precision=prec)), _bits(c))


# ------------------------------------------------------------------------------------- 5. against log_prob
def test_consistent_with_log_prob_to_second_order(dmip, golden, monkeypatch):
    """ckpt_lin, 64 chains: e(S) = max |logq_S - model.log_prob(x_S, y, 1024, precision="fp32")| at S = 32 and 64
    has a ratio in [3, 5] (two second-order discretisations of one integral), and each e(S) is within twice the f64
    restatement's own value on the same rows. (flow_ref's contractions through numpy's BLAS path: the same sums in
    another order, far faster.)"""
    monkeypatch.setattr(np, "einsum", functools.partial(np.einsum, optimize=True))
    m = _lin(dmip, golden)
    params = HR.params_of(m.sde.a)
    y = golden("flow_logp.npz")["a_y"]
    x0 = HR.x0_of_seed(1234, 64, 2)
    e_gpu, e_ref = {}, {}
    for S in (32, 64):
        x, logq = m.sample_with_log_prob(_dev(y), 64, S, x0=_dev(x0), precision=X3)
        logp = m.log_prob(x, _dev(y), num_steps=1024, precision="fp32")
        e_gpu[S] = (logq.double() - logp.double()).abs().max().item()
        x64, l64 = FS.sample_with_logq(params, x0, y, S)
        e_ref[S] = np.abs(l64 - FR.log_prob(params, x64, y, 1024)[0]).max()
    print(f"X3ORDER e_gpu = {e_gpu}, f64 restatement {e_ref}; ratio {e_gpu[32] / e_gpu[64]:.2f}")
    assert 3.0 <= e_gpu[32] / e_gpu[64] <= 5.0, e_gpu
    for S in (32, 64):
        assert e_gpu[S] <= 2 * e_ref[S], (S, e_gpu, e_ref)


# ------------------------------------------------------------------------------------- 6. range
def test_a_row_beyond_the_split_range_raises(dmip, golden):
    """One row at |x| = 1e5 > 65504: precision="fp32x3" raises "fp16 range" (the device status word, read by
    parallel.guarded); the same rows at the default precision return a finite or -inf value without raising."""
    m = _lin(dmip, golden)
    z = golden("flow_logp.npz")
    x = z["a_x"][:9].copy()
    x[4] = (1e5, -1e5)
    y = _dev(z["a_y"])
    with pytest.raises(RuntimeError, match="fp16 range"):
        m.log_prob(_dev(x), y, num_steps=4, precision=X3)
    logp = m.log_prob(_dev(x), y, num_steps=4).cpu().numpy()
    assert not np.any(np.isnan(logp)) and not np.any(logp == np.inf)
    assert np.all(np.isfinite(np.delete(logp, 4)))
    # the status word is clear again: the rows in range go through
    ok = m.log_prob(_dev(np.delete(x, 4, axis=0)), y, num_steps=4, precision=X3)
    assert torch.isfinite(ok).all()
    with pytest.raises(RuntimeError, match="fp16 range"):
        m.sample_with_log_prob(y, 9, 4, x0=_dev(x), precision=X3)


# ------------------------------------------------------------------------------------- 7. importance_posterior
def test_importance_posterior_on_the_linear_problem(dmip, golden, ev):
    """ckpt_lin against the analytic Gaussian posterior, 4,096 chains, S = 64, precision="fp32x3": every field equals
    an f64 numpy recomputation from the returned (x, logq) to 1e-9; ess_frac, log_z and the reverse KL differ from
    the exact-f32 run at the same seed by at most twice the spread of three exact-f32 seeds."""
    m = _lin(dmip, golden)
    y = _dev(golden("flow_lmbd.npz")["lin_S10_y"])
    post = dmip.LinearForwardProblem().get_posterior(y.cpu(), device="cpu")
    log_target = lambda x: post.log_prob(x.cpu())  # noqa: E731 -- (the drivers' way: the 2 x 2 Gaussian on the host)
    before = dmip._lib.calls.get("flow_sample", 0)
    rep = ev.importance_posterior(m, y, log_target, 4096, 64, seed=7, precision=X3)
    assert dmip._lib.calls["flow_sample"] == before + 1
    x, logq = rep["x"], rep["logq"]
    assert tuple(x.shape) == (4096, 2) and tuple(logq.shape) == (4096,) and x.is_cuda
    xs, lq = x.cpu().numpy().astype(np.float64), logq.cpu().numpy().astype(np.float64)
    lw = log_target(x).numpy().astype(np.float64) - lq
    w = np.exp(lw - lw.max())
    ess, log_z = w.sum() ** 2 / (w * w).sum(), np.log(w.mean()) + lw.max()
    wn = w / w.sum()
    mean = (wn[:, None] * xs).sum(0)
    cov = np.einsum("n,ni,nj->ij", wn, xs - mean, xs - mean)
    rel = lambda a, b: np.abs(np.asarray(a) - np.asarray(b)).max() / max(1.0, np.abs(np.asarray(b)).max())  # noqa: E731
    assert rel(rep["ess"], ess) <= 1e-9 and rel(rep["ess_frac"], ess / 4096) <= 1e-9
    assert rel(rep["log_z"], log_z) <= 1e-9 and rel(rep["reverse_kl"], -lw.mean() + log_z) <= 1e-9
    assert rel(rep["weights"], wn) <= 1e-9 and rel(rep["mean"], xs.mean(0)) <= 1e-9
    assert rel(rep["snis_mean"], mean) <= 1e-9 and rel(rep["snis_cov"], cov) <= 1e-9
    assert 0.0 < rep["ess_frac"] <= 1.0 and np.isfinite(rep["log_z"])
    f32 = [ev.importance_posterior(m, y, log_target, 4096, 64, seed=s, precision="fp32") for s in (7, 8, 9)]
    for k in ("ess_frac", "log_z", "reverse_kl"):
        v = [r[k] for r in f32]
        spread = max(v) - min(v)
        print(f"X3IMPORTANCE {k}: fp32x3 {rep[k]:.6f}, fp32 (seeds 7, 8, 9) {v[0]:.6f} {v[1]:.6f} {v[2]:.6f}, "
              f"|fp32x3 - fp32| = {abs(rep[k] - v[0]):.3e}, spread {spread:.3e}")
        assert abs(rep[k] - v[0]) <= 2 * spread, (k, rep[k], v)
