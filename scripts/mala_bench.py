"""The fused Metropolis-adjusted Langevin sampler on one MI355X (dmip_mala_sample, csrc/dmip_surrogate.hip mala_kernel).

  * Timing, HIP events, median of --reps, the three paths alternated rep by rep at the same shape (--chains chains x
    --steps steps x 1 y, one Langevin sub-step per step):
      fused    one launch of mala_kernel for all steps;
      rw       (a) the exact-f32 random-walk kernel (dmip_mh_sample): one forward pass per step where MALA runs a forward
               and a reverse pass, NCF = 34 ring chunks against NCF + NCB = 66;
      unfused  (b) the same scheme as --unfused-steps iterations of dmip_log_posterior with its gradient plus the torch
               update (randn, proposal, log proposal ratio, rand, select), scaled to --steps.
    ms per step, chain-evaluations/s (one evaluation = forward + reverse pass = 2 x 275,456 algorithmic flop) and the
    fraction of the f32 MFMA peak.
  * Same-shape comparison from the random-walk chains' final states on the fixture y: the accept share and the
    per-dimension lag-50 autocorrelation over chains (corr of x_t and x_{t+50}) of MALA at stepsize 1e-3 and 5e-3
    beside the random walk at noise_std 0.5.
Prints one JSON line and writes it to --out.   python scripts/mala_bench.py [--out profiles/mala/mala_bench.json]"""
import argparse
import importlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FLOPS_EVAL = 2 * (3 * 256 + 2 * 256 * 256 + 256 * 23)  # one forward pass (scripts/bench_surrogate.py)
PEAK_F32_MFMA = 157.3  # TFLOP/s, MI355X dense f32-input MFMA


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=30000)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--unfused-steps", type=int, default=None, help="iterations of the unfused path (default --steps)")
    ap.add_argument("--stepsize", type=float, default=1e-3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--lag", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mala", "mala_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mala_bench: needs a HIP device")
    from bench_surrogate import surrogate
    pr = importlib.import_module("diffusion-modelling-for-inverse-problems_amd.problems")
    L = importlib.import_module("diffusion-modelling-for-inverse-problems_amd._lib")
    dev = torch.device("cuda:0")
    fm = surrogate(dev)
    prm = {"a": 0.2, "b": 0.01, "lambd_bd": 1000}
    y = torch.from_numpy(np.load(os.path.join(ROOT, "tests", "golden", "surrogate_io.npz"))["mh_y"])[None].to(dev)
    n, S, h = a.chains, a.steps, a.stepsize
    Su = a.unfused_steps or S
    st = torch.cuda.current_stream()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record(st)
        fn()
        e1.record(st)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    x_rw = pr.mh_sample(fm, prm, y, n, 1000, 0.5, seed=77)  # near-stationary starts for every path
    handle, nz = pr.surrogate_handle(fm, dev), L.scat_noise(0.2, 0.01, 1000)
    c = float(np.sqrt(2 * h))

    def unfused():
        x = x_rw[0].clone()
        e, g = torch.empty(n, device=dev), torch.empty(n, 3, device=dev)
        L.log_posterior(handle, nz, x, y, 0, e, g)
        for _ in range(Su):
            eta = torch.randn_like(x)
            yy = x - h * g + c * eta
            e_y, g_y = torch.empty_like(e), torch.empty_like(g)
            L.log_posterior(handle, nz, yy, y, 0, e_y, g_y)
            eta_ = (x - yy + h * g_y) / c
            ld = 0.5 * (eta ** 2 - eta_ ** 2).sum(1)
            acc = torch.rand_like(e) < torch.exp(-e_y + e + ld)
            x = torch.where(acc[:, None], yy, x)
            g = torch.where(acc[:, None], g_y, g)
            e = torch.where(acc, e_y, e)
        return x

    paths = {"fused": lambda: pr.mala_sample(fm, prm, y, n, S, h, seed=1, x_init=x_rw),
             "rw": lambda: pr.mh_sample(fm, prm, y, n, S, 0.5, seed=1, x_init=x_rw),
             "unfused": unfused}
    for fn in paths.values():
        fn()  # warm up every shape
    ms = {k: [] for k in paths}
    for _ in range(a.reps):
        for k, fn in paths.items():
            ms[k].append(timed(fn))
    med = {k: float(np.median(v)) for k, v in ms.items()}
    per_step = {"fused": med["fused"] / S, "rw": med["rw"] / S, "unfused": med["unfused"] / Su}
    evals_per_s = n / (per_step["fused"] * 1e-3)
    tf = evals_per_s * 2 * FLOPS_EVAL / 1e12

    def lag_stats(step_fn, accept_fn):
        x1 = step_fn(a.lag)
        x0c, x1c = x_rw[0].double().cpu().numpy(), x1[0].double().cpu().numpy()
        return {"accept_share": accept_fn(),
                "lag_autocorr": [float(np.corrcoef(x0c[:, d], x1c[:, d])[0, 1]) for d in range(3)]}

    def mala_accept(hh):
        _, na = pr.mala_sample(fm, prm, y, n, a.lag, hh, seed=3, x_init=x_rw, return_accept=True)
        return float(na.float().mean().item() / a.lag)

    def rw_accept():  # the share of chains that one step moves
        x1 = pr.mh_sample(fm, prm, y, n, 1, 0.5, seed=4, x_init=x_rw)
        return float((x1 != x_rw).any(dim=2).float().mean().item())

    mixing = {f"mala_stepsize_{hh:g}": lag_stats(lambda k, hh=hh: pr.mala_sample(fm, prm, y, n, k, hh, seed=3, x_init=x_rw),
                                                 lambda hh=hh: mala_accept(hh)) for hh in (1e-3, 5e-3)}
    mixing["random_walk_noise_std_0.5"] = lag_stats(lambda k: pr.mh_sample(fm, prm, y, n, k, 0.5, seed=3, x_init=x_rw),
                                                    rw_accept)
    out = {
        "metric": "fused MALA chain-evaluations/s (scatterometry surrogate, forward + reverse pass)",
        "value": evals_per_s, "unit": "chain-evaluations/s",
        "config": {"chains": n, "steps": S, "lang_steps": 1, "stepsize": h, "n_y": 1, "reps": a.reps,
                   "unfused_steps": Su},
        "ms_per_launch": {k: v for k, v in ms.items()}, "ms_median": med, "ms_per_step": per_step,
        "roofline": {"bound": "mfma", "achieved": tf, "peak": PEAK_F32_MFMA, "unit": "TFLOP/s",
                     "frac": tf / PEAK_F32_MFMA, "dtype": "f32 (v_mfma_f32_16x16x4_f32)",
                     "flops_per_chain_evaluation": 2 * FLOPS_EVAL},
        "ratio_fused_over_rw": per_step["fused"] / per_step["rw"],
        "ratio_unfused_over_fused": per_step["unfused"] / per_step["fused"],
        "mixing": {"lag": a.lag, "start": "final states of 1000 random-walk steps", **mixing},
    }
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
