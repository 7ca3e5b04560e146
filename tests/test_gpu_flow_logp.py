"""model.log_prob: the fused probability-flow log-likelihood kernel (csrc/dmip_flow.hip, dmip_flow_logp) against the
reference's own evaluation (tests/golden/flow_logp.npz) and the f64 restatement (tests/flow_ref.py). Needs an
MI355X: `pytest -m gpu`.

Gate of every accuracy test (flow_gpu.gate; tests/flow_cases.py derives it): with e_gpu = max |logp_gpu - logp_f64| and
e_cpu = max |logp_f32_cpu - logp_f64| (the same scheme evaluated in f32 on the CPU: the reference's own f32 arithmetic
for the fixture cases, flow_ref's f32 run for the shapes without a fixture), e_gpu <= 8 max(e_cpu, 1e-7) and never
above the gate it replaced, 4 e_cpu + 1e-6 (the smaller of the two wherever e_cpu > 2.5e-7). The latent x_S gets the
same gate. For the seeded shapes there is one f64 and one f32 run of flow_ref per network, shared and sliced by the
ragged cases; e_gpu and e_cpu are taken over the same rows.
"""
import numpy as np
import pytest
import torch

import flow_ref as FR
import oracle as O
from flow_gpu import DEV, gate, lin, post, scat, seeded

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def _gate(name, got, ref64, ref32):
    gate(name, got, ref64, ref32, scaled=False, tag="F32GATE ")  # (the replaced gate's additive term: 1e-6)


def _fixture_model(dmip, golden, case):
    return {"a": lin, "c": lin, "b": scat, "d": post}[case](dmip, golden)


@pytest.mark.parametrize("case", ["a", "b", "d"])
def test_fixture_parity(dmip, golden, case):
    """Cases (a) ckpt_lin 37 rows S = 20, (b) ckpt_scat 50 rows S = 10, (d) the Posterior pair, 21 rows x 2 ys, S = 6
    (measured e_gpu / e_cpu: DESIGN.md, "Probability-flow ODE")."""
    z = golden("flow_logp.npz")
    m = _fixture_model(dmip, golden, case)
    before = dmip._lib.calls.get("flow_logp", 0)
    logp, lat = m.log_prob(torch.from_numpy(z[f"{case}_x"]).to(DEV), torch.from_numpy(z[f"{case}_y"]).to(DEV),
                           num_steps=int(z[f"{case}_S"]), return_latent=True)
    assert dmip._lib.calls["flow_logp"] == before + 1
    assert logp.dtype == torch.float32 and logp.is_cuda
    assert tuple(logp.shape) == z[f"{case}_logp_f64"].shape and tuple(lat.shape) == z[f"{case}_x"].shape
    _gate(f"({case}) logp", logp.cpu().numpy().astype(np.float64), z[f"{case}_logp_f64"], z[f"{case}_logp_f32_cpu"])
    _gate(f"({case}) latent", lat.cpu().numpy().astype(np.float64), z[f"{case}_latent_f64"],
          z[f"{case}_latent_f32_cpu"].astype(np.float64))


# ------------------------------------------------------------------ seeded shapes against flow_ref
SHAPES = {  # name: (W, n_hidden, xdim, ydim, rows of the shared reference, S, weight seed)
    "w64": (64, 3, 2, 2, 37, 6, 301),
    "w128": (128, 3, 2, 2, 19, 6, 302),
    "w512x1": (512, 1, 3, 23, 21, 6, 303),
    "w512x3": (512, 3, 3, 23, 21, 6, 304),
}
_refs = {}


def _seeded(dmip, name):
    """(model, x (n, d), ys (3, ydim), S, per-y (logp_f64, latent_f64, logp_f32, latent_f32)) -- the reference is
    computed once per shape and shared, unchanged, by the tests that slice it."""
    W, NL, xd, yd, n, S, seed = SHAPES[name]
    m, params = seeded(dmip, W, NL, xd, yd, seed)
    if name not in _refs:
        g = np.random.default_rng(seed)
        x = g.normal(size=(n, xd)).astype(np.float32)
        ys = g.normal(size=(3, yd)).astype(np.float32)
        n_y = 3 if name == "w64" else 1
        ref = []
        for i in range(n_y):
            l64, z64 = FR.log_prob(params, x, ys[i], S)
            l32, z32 = FR.log_prob(params, x, ys[i], S, dtype=np.float32)
            for a in (l64, z64, l32, z32):
                a.setflags(write=False)
            ref.append((l64, z64, l32, z32.astype(np.float64)))
        _refs[name] = (x, ys, ref)
    x, ys, ref = _refs[name]
    return m, x, ys, S, ref


@pytest.mark.parametrize("name,n", [("w64", 1), ("w64", 3), ("w64", 5), ("w64", 17), ("w64", 37), ("w128", 19),
                                    ("w512x1", 21), ("w512x3", 21)])
def test_ragged_rows_vs_flow_ref(dmip, name, n):
    """Row counts that are no multiple of the 4-row pass or of a workgroup's rows, every compiled width class and
    both depths of the wide network (1 hidden layer: no streamed hidden tile at all)."""
    m, x, ys, S, ref = _seeded(dmip, name)
    l64, z64, l32, z32 = ref[0]
    logp, lat = m.log_prob(torch.from_numpy(x[:n]).to(DEV), torch.from_numpy(ys[0]).to(DEV), num_steps=S,
                           return_latent=True)
    assert tuple(logp.shape) == (n,) and tuple(lat.shape) == (n, x.shape[1])
    _gate(f"{name} n={n} logp", logp.cpu().numpy(), l64[:n], l32[:n])
    _gate(f"{name} n={n} latent", lat.cpu().numpy(), z64[:n], z32[:n])


def test_multi_y(dmip):
    """n_y = 3, a different y each: every y index reads its own layer-1 image."""
    m, x, ys, S, ref = _seeded(dmip, "w64")
    n = 5
    xs = np.stack([x[:n], x[7:7 + n], x[20:20 + n]])
    logp = m.log_prob(torch.from_numpy(xs).to(DEV), torch.from_numpy(ys).to(DEV), num_steps=S).cpu().numpy()
    assert logp.shape == (3, n)
    for i, lo in enumerate((0, 7, 20)):
        l64, _, l32, _ = ref[i]
        _gate(f"multi-y {i} logp", logp[i], l64[lo:lo + n], l32[lo:lo + n])
    assert np.abs(logp[0] - ref[1][0][:n]).max() > 1e-3  # the ys do differ


@pytest.mark.parametrize("r", [0, 3, 4, 16, 36])
def test_row_independence_bitwise(dmip, r):
    """The log-density of row r is bitwise the same alone or among 37 rows (quad / column cross-talk in the DPP
    broadcast or the output shuffles would show here)."""
    m, x, ys, S, _ = _seeded(dmip, "w64")
    y = torch.from_numpy(ys[0]).to(DEV)
    full, lat = m.log_prob(torch.from_numpy(x).to(DEV), y, num_steps=S, return_latent=True)
    one, lat1 = m.log_prob(torch.from_numpy(x[r:r + 1]).to(DEV), y, num_steps=S, return_latent=True)
    np.testing.assert_array_equal(one.cpu().numpy().view(np.uint32), full[r:r + 1].cpu().numpy().view(np.uint32))
    np.testing.assert_array_equal(lat1.cpu().numpy().view(np.uint32), lat[r:r + 1].cpu().numpy().view(np.uint32))


def test_density_normalises_on_the_grid(dmip, golden):
    """Case (c): ckpt_lin on the 48 x 48 grid of half-width 3 around the posterior mean, S = 50: the grid integral
    of exp(logp) equals the reference's (1.0024) to 1e-4 relative; no NaN or inf on the grid."""
    z = golden("flow_logp.npz")
    m = _fixture_model(dmip, golden, "c")
    logp = m.log_prob(torch.from_numpy(z["c_x"]).to(DEV), torch.from_numpy(z["c_y"]).to(DEV),
                      num_steps=int(z["c_S"])).cpu().numpy().astype(np.float64)
    assert logp.shape == (48 * 48,) and np.all(np.isfinite(logp))
    integral = np.exp(logp).sum() * float(z["c_cell"])
    print(f"grid integral {integral:.6f} (reference {float(z['c_integral']):.6f})")
    assert abs(integral - float(z["c_integral"])) <= 1e-4 * float(z["c_integral"])
    _gate("(c) logp", logp, z["c_logp_f64"], z["c_logp_f32_cpu"])


def test_round_trip_through_the_sampler(dmip, golden):
    """x -> latent (Heun, log_prob) -> x (the sampler's Euler steps at lmbd = 1, the latent injected as x0), 200
    steps each way. The integrators differ by construction: the gate is twice the mismatch flow_ref's f64 round
    trip has on the same rows (the measurement; the factor 2 covers f32 rounding)."""
    z = golden("flow_logp.npz")
    m = _fixture_model(dmip, golden, "a")
    params = O.mlp_params_from_state(golden("ckpt_lin.npz"))
    x, y, S = z["a_x"], z["a_y"], 200
    _, lat64 = FR.log_prob(params, x, y, S)
    ref_err = np.abs(FR.ode_sample(params, lat64, y, S) - x).max()
    _, lat = m.log_prob(torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV), num_steps=S, return_latent=True)
    noise = torch.zeros(S + 1, 1, x.shape[0], 2, device=DEV)
    noise[0, 0] = lat
    back = m.sample_device(torch.from_numpy(y).to(DEV), x.shape[0], S, mean=0, std=1, noise=noise, precision="fp32",
                           lmbd=1.0)[0].cpu().numpy()
    err = np.abs(back - x).max()
    print(f"round trip: max |x_back - x| = {err:.3e} (f64 restatement {ref_err:.3e})")
    assert np.all(np.isfinite(back)) and err <= 2 * ref_err, (err, ref_err)


def test_refusals_launch_nothing(dmip):
    """A width without a kernel (96, through the eager MLP) and a SiLU network raise before any launch."""
    x, y = torch.zeros(4, 3, device=DEV), torch.zeros(23, device=DEV)
    m96 = dmip.CDE(3, 23, [96] * 3)
    silu = dmip.CDE(3, 23, [256] * 3)
    silu.sde.a = dmip.MLP(3 + 23 + 1, 3, [256] * 3, torch.nn.SiLU()).to(DEV)
    for m in (m96, silu):
        before = dict(dmip._lib.calls)
        with pytest.raises(ValueError):
            m.log_prob(x, y, num_steps=4)
        assert dict(dmip._lib.calls) == before
    with pytest.raises(ValueError):
        dmip.CDiffE(3, 23, [256] * 3).log_prob(x, y)
