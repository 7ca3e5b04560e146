"""Every fused fp32 and fp32x3 sampler held to f32 accuracy against float64 (tests/accuracy_cases.py): the kernel's
element-wise error against the float64 restatement of the same chains is at most K = 8 times the f32 oracle's own
(floor 1e-7). Needs an MI355X: `pytest -m gpu`; `-s` prints every case's e_gpu, e_cpu and ratio (DESIGN.md 3c lists
them). tests/test_accuracy_host.py proves on the CPU that a kernel with one of its three products lost, its lo
subnormals flushed or its activations in fp16 would miss this gate by 4x or more on every case here.

Each test is one launch of at most 700 chains x 200 steps. The older, coarser gates stand beside this one.
"""
import importlib

import numpy as np
import pytest
import torch

import accuracy_cases as A
import sde_cases

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def _launch_key(c):
    if c.kind.startswith("heun"):
        return "ode_sample"
    if c.extra.get("lmbd"):
        return "em_sample_lmbd"
    return {"cde": "em_sample", "post": "em_sample_posterior", "cdiffe": "em_sample_cdiffe"}[c.kind]


def _sample(dmip, cid, S, prec, m=None, y=None, x0=None, n=None, chain_offset=0):
    """The case's chains [chain_offset, chain_offset + n) from the fused kernel of `prec`, as numpy (n, xdim)."""
    c = A.case(cid)
    if m is None:
        m, _, _, y, x0 = A.model(dmip, cid)
        sde_cases.set_sde(dmip, m, c.sde)
    n = c.n if n is None else n
    est = importlib.import_module(dmip.__name__ + ".estimators")
    L = dmip._lib
    mode = {"cde": L.DMIP_SAMPLER_CDE, "post": L.DMIP_SAMPLER_POSTERIOR, "cdiffe": L.DMIP_SAMPLER_CDIFFE}[
        c.kind.replace("heun-", "")]
    solver = "heun" if c.kind.startswith("heun") else "euler"
    # the requested engine itself, not the next more accurate one
    assert est._fused_precision(prec, mode, c.W, c.NL, c.xd, c.yd, solver=solver) == prec
    kw = dict(c.extra)
    if solver == "heun":
        kw.update(solver="heun", x0=torch.from_numpy(np.array(x0[chain_offset:chain_offset + n])))
    key = _launch_key(c)
    before = L.calls.get(key, 0)
    out = m.sample_device(torch.from_numpy(np.array(y)).to(DEV), n, S, seed=A.SEED, chain_offset=chain_offset,
                          precision=prec, **kw)
    assert L.calls[key] == before + 1  # the fused launch ran, not the per-step loop
    L.device_status(out.device)
    return out[0].cpu().numpy()


@pytest.mark.parametrize("cid,S,prec", A.DEVICE_RUNS)
def test_sampler_holds_f32_accuracy(dmip, monkeypatch, cid, S, prec):
    for k, v in A.CASES[cid].env.items():
        monkeypatch.setenv(k, v)
    got = _sample(dmip, cid, S, prec)
    A.gate(dmip, cid, S, got, tag=f" {prec}")


@pytest.mark.parametrize("cid", A.SHARDS)
def test_shards_are_the_whole_run_at_50_steps(dmip, cid):
    """Two chain_offset shards equal the whole run bit for bit over 50 steps (the engines' own shard tests run 6 to
    10), the split inside the first tile."""
    c = A.CASES[cid]
    m, _, _, y, _ = A.model(dmip, cid)
    sde_cases.set_sde(dmip, m, c.sde)
    cut = 13
    full = _sample(dmip, cid, A.SHARD_STEPS, "fp32x3", m, y)
    lo = _sample(dmip, cid, A.SHARD_STEPS, "fp32x3", m, y, n=cut)
    hi = _sample(dmip, cid, A.SHARD_STEPS, "fp32x3", m, y, n=c.n - cut, chain_offset=cut)
    assert np.all(np.isfinite(full))
    np.testing.assert_array_equal(np.concatenate([lo, hi]).view(np.uint32), full.view(np.uint32))
