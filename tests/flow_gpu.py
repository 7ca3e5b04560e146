"""What the GPU tests of the flow kernels share (test_gpu_flow_logp.py, test_gpu_flow_sample.py, test_gpu_flow_x3.py):
the accuracy gate (flow_cases.py's), the fixture and seeded models, and the device-side helpers. A plain module beside
flow_ref.py."""
import numpy as np
import torch

import flow_cases as FC
import flow_sample_ref as FS
import oracle as O
from conftest import state_from_npz

DEV = "cuda:0"


def bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint32)


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)  # (a copy: the shared references are read-only)


def gate(name, got, ref64, ref32, scaled=True, tag=""):
    """flow_cases.gate, every flow test's: e_gpu <= K max(e_cpu, 1e-7), K = 8 (flow_cases.CASE_K by `name`), with
    e_gpu = max |gpu - f64| and e_cpu = max |f32 restatement - f64| over the same rows, and never above the gate it
    replaced, 4 e_cpu + 1e-6 max(1, max |f64|) (`scaled`; else + 1e-6). flow_cases.py derives K."""
    FC.gate(name, got, ref64, ref32, scaled=scaled, tag=tag)


def load_linear(net, params):
    lins = [m for m in net if isinstance(m, torch.nn.Linear)]
    assert len(lins) == len(params)
    with torch.no_grad():
        for lin, (W, b) in zip(lins, params):
            lin.weight.copy_(torch.from_numpy(W))
            lin.bias.copy_(torch.from_numpy(b))


def seeded(dmip, W, NL, xd, yd, seed):
    """(CDE model, its params) with oracle.reference_weights of `seed`: the network of every seeded shape."""
    params = O.reference_weights([xd + yd + 1] + [W] * NL + [xd], seed)
    m = dmip.CDE(xd, yd, [W] * NL)
    load_linear(m.sde.a, params)
    return m, params


def lin(dmip, golden):
    m = dmip.CDE(2, 2, [64] * 3)
    m.sde.a.load_state_dict(state_from_npz(golden("ckpt_lin.npz")))
    return m


def scat(dmip, golden):
    m = dmip.CDE(3, 23, [256] * 3)
    m.sde.a.load_state_dict(state_from_npz(golden("ckpt_scat.npz")))
    return m


def post(dmip, golden):
    m = dmip.PosteriorDiffusionEstimator(3, 23, [256] * 3)
    m.sde.a.prior_net.load_state_dict(state_from_npz(golden("ckpt_prior_scat.npz")))
    m.sde.a.likelihood_net.load_state_dict(state_from_npz(golden("posterior_loss.npz"), "lik_"))
    return m


def case_model(dmip, golden, cid):
    """The model of a flow_cases case (its paired form shares the network)."""
    name = FC.PAIRED.get(cid, cid)
    if name in FC.SHAPES:
        W, NL, xd, yd, _, seed = FC.SHAPES[name]
        return seeded(dmip, W, NL, xd, yd, seed)[0]
    return {"a": lin, "b": scat, "d": post}[name](dmip, golden)


def sample_reference(params, x0, y, S, prior=None):
    """((x_f64, logq_f64), (x_f32, logq_f32)) of the restatement, read-only."""
    out = []
    for dtype in (np.float64, np.float32):
        x, lq = FS.sample_with_logq(params, x0, y, S, prior, dtype=dtype)
        x.setflags(write=False), lq.setflags(write=False)
        out.append((x, lq))
    return out


def device_x0(dmip, seed, offset, stream, n, xd, mean=0.0, std=1.0):
    """mean + std times the first xd normals of each chain's stream, from the device's own generator."""
    pairs = (xd + 1) // 2
    out = torch.empty(n, 2 * pairs, device=DEV, dtype=torch.float32)
    dmip._lib.rng_normals(seed, offset, stream, n, pairs, out)
    torch.cuda.synchronize()
    f = lambda v: torch.tensor(v, device=DEV, dtype=torch.float32)  # noqa: E731
    return (out[:, :xd] * f(std) + f(mean)).contiguous()
