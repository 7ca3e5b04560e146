"""What the stochastic few-step samplers cost and how their draws are distributed: 100,000 chains of the
scatterometry CDE [256]^3 (tests/golden/ckpt_scat.npz), one y, fp32x3, timed by HIP events, median of --reps, in one
session --
  * solver="dpm2m" at eta = 1 (SDE-DPM-Solver++(2M); the one-tile engine, csrc/dmip_x3.h SOLVER_TABLE_SDE) at 32 / 64 /
    128 network evaluations, and "ddim" at eta = 1 (ancestral sampling) at 128;
  * the same at eta = 0 (the deterministic kernels, SOLVER_TABLE) and the one-tile engine's Euler-Maruyama kernel
    (DMIP_X3K=0, the reverse SDE: one draw per step) at as many evaluations, with the ratio of the time per
    chain-evaluation to each: the stochastic step is the deterministic one plus Euler's draw;
  * KS and sliced W1 of every run's draws against Euler-Maruyama at 1000 steps from the same model on its default engine
    (an independent sample: another seed), among them "dpm2m" at eta = 0 and Euler at 128 steps for comparison.
One JSON line.
    python scripts/multistep_sde_bench.py [--chains 100000] [--reps 3] [--out FILE]"""
import argparse
import importlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from heun_bench import timed  # noqa: E402

EVALS = (32, 64, 128)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    pkg = importlib.import_module("diffusion-modelling-for-inverse-problems_amd")
    metrics = importlib.import_module("diffusion-modelling-for-inverse-problems_amd.metrics")
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream(dev)
    n, seed, prec = a.chains, a.seed, "fp32x3"
    m = pkg.CDE(3, 23, [256] * 3)
    z = np.load(os.path.join(ROOT, "tests", "golden", "ckpt_scat.npz"))
    m.sde.a.load_state_dict({k: torch.from_numpy(z[k.replace(".", "_")]) for k in m.sde.a.state_dict()}, strict=True)
    m.sde.a.to(dev)
    ys = np.load(os.path.join(ROOT, "tests", "golden", "samples_scat.npz"))["y"].astype(np.float32)
    y = torch.from_numpy(ys).to(dev)

    # the yardstick: the reverse SDE by Euler-Maruyama at 1000 steps, other chains (seed + 1) of the same model
    ref = m.sample_device(y, n, 1000, seed=seed + 1, precision=prec)[0].double().cpu().numpy()
    pkg._lib.device_status(dev)

    def dist(x):
        rep = metrics.parity_report(x[0].double().cpu().numpy(), ref)
        return {"ks_max": max(rep["ks_draws"]["stat"]), "ks_crit": rep["ks_draws"]["crit"],
                "sliced_w1": rep["sliced_w1_draws"]["stat"], "sliced_w1_null": rep["sliced_w1_draws"]["null"],
                "finite": bool(torch.isfinite(x).all())}

    def run(S, engine, **kw):
        ms, all_ms, x = timed(lambda: m.sample_device(y, n, S, seed=seed, precision=prec, **kw), a.reps, st)
        return dict(ms=ms, ms_runs=all_ms, network_evals=S, ns_per_chain_eval=ms * 1e6 / (n * S), engine=engine, **dist(x))

    out = {"chains": n, "hidden_layers": [256] * 3, "precision": prec, "device": torch.cuda.get_device_name(0),
           "reps": a.reps, "grid": "logsnr", "t_end": 1e-3,
           "ref": "Euler-Maruyama, 1000 steps, seed + 1 (the default engine)"}
    calls = pkg._lib.calls
    runs = {}
    before = calls["multistep_sde_sample"]
    for S in EVALS:
        runs[f"dpm2m_eta1_{S}"] = run(S, "x3 (one tile), SOLVER_TABLE_SDE", solver="dpm2m", eta=1.0)
    runs["ddim_eta1_128"] = run(128, "x3 (one tile), SOLVER_TABLE_SDE", solver="ddim", eta=1.0)
    assert calls["multistep_sde_sample"] == before + 4 * (a.reps + 1)
    for S in EVALS:
        runs[f"dpm2m_eta0_{S}"] = run(S, "x3 (one tile), SOLVER_TABLE", solver="dpm2m")
    runs["euler_1000"] = run(1000, "x3k (k-major, the default)")
    os.environ["DMIP_X3K"] = "0"  # the one-tile engine's Euler-Maruyama kernel, at as many evaluations
    for S in EVALS:
        runs[f"euler_{S}_x3"] = run(S, "x3 (one tile), Euler-Maruyama")
    del os.environ["DMIP_X3K"]
    pkg._lib.device_status(dev)
    out["runs"] = runs
    for S in EVALS:
        t = runs[f"dpm2m_eta1_{S}"]["ns_per_chain_eval"]
        out[f"eta1_vs_eta0_per_eval_{S}"] = t / runs[f"dpm2m_eta0_{S}"]["ns_per_chain_eval"]
        out[f"eta1_vs_x3_euler_per_eval_{S}"] = t / runs[f"euler_{S}_x3"]["ns_per_chain_eval"]
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
