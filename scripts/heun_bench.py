"""What the second-order ODE sampler is worth in wall time: 100,000 chains of the scatterometry CDE
[256]^3 (tests/golden/ckpt_scat.npz), one y, fp32x3, timed by HIP events --
  * solver="heun" at S = 128 and S = 256 (the one-tile engine, csrc/dmip_x3.h) beside the lmbd = 1 Euler sampler at
    S = 1000 on its default engine (the k-major one, csrc/dmip_x3k.h), all from the same x0 (one seed);
  * each run's distance to the f64 Heun-2048 reference from that x0: max and median per-chain error, and the
    per-dimension KS / W1 and sliced W1 of metrics.parity_report. The reference is the scheme of tests/heun_ref.py
    in eager torch float64 on the device (a yardstick, not a product path);
  * the time per network evaluation of the one-tile engine's Heun kernel against its Euler kernel (DMIP_X3K=0) at as
    many evaluations (S = 128 Heun, S = 256 Euler): the second stage is a second call of the same evaluation, so
    about 1x is expected.
One JSON line.
    python scripts/heun_bench.py [--chains 100000] [--reps 3] [--ref-steps 2048] [--out FILE]"""
import argparse
import importlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, reps, st):
    fn()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        out = fn()
        e1.record(st)
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts)), [float(t) for t in ts], out


def heun_f64(net, x0, y, S, T=1.0, bmin=0.1, bmax=20.0):
    """The scheme of csrc/dmip_device.h HeunStep in float64 (tau: the kernels' f32 grid), eager torch."""
    lin = [m for m in net if isinstance(m, torch.nn.Linear)]
    W = [m.weight.detach().double() for m in lin]
    b = [m.bias.detach().double() for m in lin]
    ts = (torch.linspace(0, 1, S + 1) * T).float()
    tau = (T - ts).double().tolist()
    x = x0.double()
    yy = y.double().reshape(1, -1).expand(x.shape[0], -1)

    def slope(x, t):
        h = torch.cat([x, yy, torch.full((x.shape[0], 1), t, dtype=torch.float64, device=x.device)], 1)
        h = torch.tanh(torch.tanh(h @ W[0].T + b[0]))
        for Wl, bl in zip(W[1:-1], b[1:-1]):
            h = torch.tanh(h @ Wl.T + bl)
        a = h @ W[-1].T + b[-1]
        beta = bmin + (bmax - bmin) * t
        return 0.5 * beta ** 0.5 * a + 0.5 * beta * x

    d = T / S
    for i in range(S):
        k1 = slope(x, tau[i])
        k2 = slope(x + d * k1, tau[i + 1])
        x = x + (0.5 * d) * (k1 + k2)
    return x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--ref-steps", type=int, default=2048)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    pkg = importlib.import_module("diffusion-modelling-for-inverse-problems_amd")
    est = importlib.import_module("diffusion-modelling-for-inverse-problems_amd.estimators")
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

    # the chains' own x0: the first normals of stream (seed, chain, y index 0)
    x0 = est._loop_normals(seed, 0, 0, n, 3, dev).contiguous()
    ref = heun_f64(m.sde.a, x0, y, a.ref_steps)
    torch.cuda.synchronize()
    ref_np = ref.cpu().numpy()

    def dist(x):
        x = x[0].double()
        e = (x - ref).abs().amax(1)
        rep = metrics.parity_report(x.cpu().numpy(), ref_np)
        return {"max_abs_err": float(e.max()), "median_chain_err": float(e.median()),
                "ks_max": max(rep["ks_draws"]["stat"]), "ks_crit": rep["ks_draws"]["crit"],
                "w1_max": max(rep["w1_draws"]["stat"]), "w1_null_min": min(rep["w1_draws"]["null"]),
                "sliced_w1": rep["sliced_w1_draws"]["stat"], "sliced_w1_null": rep["sliced_w1_draws"]["null"],
                "parity_pass": rep["pass"]}

    out = {"chains": n, "hidden_layers": [256] * 3, "precision": prec, "ref": f"f64 Heun-{a.ref_steps} (eager torch)",
           "device": torch.cuda.get_device_name(0), "reps": a.reps}
    runs = {}
    for S in (128, 256):
        ms, all_ms, x = timed(lambda: m.sample_device(y, n, S, seed=seed, precision=prec, solver="heun"), a.reps, st)
        runs[f"heun_{S}"] = dict(ms=ms, ms_runs=all_ms, network_evals=2 * S, ns_per_chain_eval=ms * 1e6 / (n * 2 * S),
                                 engine="x3 (one tile)", **dist(x))
        if S == 128:
            xi = m.sample_device(y, n, S, precision=prec, solver="heun", x0=x0)
            out["x0_is_the_stream_s_first_draw"] = bool(torch.equal(xi, x))
    ms, all_ms, x = timed(lambda: m.sample_device(y, n, 1000, seed=seed, precision=prec, lmbd=1.0), a.reps, st)
    runs["euler_1000"] = dict(ms=ms, ms_runs=all_ms, network_evals=1000, ns_per_chain_eval=ms * 1e6 / (n * 1000),
                              engine="x3k (k-major, the default)", **dist(x))
    os.environ["DMIP_X3K"] = "0"  # the one-tile engine's Euler kernel, at as many evaluations as Heun-128
    ms, all_ms, x = timed(lambda: m.sample_device(y, n, 256, seed=seed, precision=prec, lmbd=1.0), a.reps, st)
    del os.environ["DMIP_X3K"]
    runs["euler_256_x3"] = dict(ms=ms, ms_runs=all_ms, network_evals=256, ns_per_chain_eval=ms * 1e6 / (n * 256),
                                engine="x3 (one tile)", **dist(x))
    pkg._lib.device_status(dev)
    out["runs"] = runs
    out["heun_128_vs_euler_1000_time"] = runs["euler_1000"]["ms"] / runs["heun_128"]["ms"]
    out["heun_256_vs_euler_1000_time"] = runs["euler_1000"]["ms"] / runs["heun_256"]["ms"]
    out["x3_heun_per_eval_vs_x3_euler_per_eval"] = runs["heun_128"]["ns_per_chain_eval"] / \
        runs["euler_256_x3"]["ns_per_chain_eval"]
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
