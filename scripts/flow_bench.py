"""model.log_prob throughput (csrc/dmip_flow.hip) at the reference evaluation's size -- 30,000 rows, 200 Heun steps,
the scatterometry CDE at [256]^3 (tests/golden/ckpt_scat.npz) and at the reference width [512]^3 (random init) --
timed by HIP events, next to the exact-f32 CDE sampler on the same device (the same engine and MFMA work per
column). A row costs 2 S (1 + xdim) network column-evaluations; the roofline fraction counts 2 * weights flops per
column-evaluation against the f32 MFMA peak. One JSON line.
    python scripts/flow_bench.py [--rows 30000] [--steps 200] [--reps 3]"""
import argparse
import importlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
F32_MFMA_PEAK = 157.3e12  # v_mfma_f32_16x16x4_f32, MI355X


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
    return float(np.median(ts)), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=30000)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    pkg = importlib.import_module("diffusion-modelling-for-inverse-problems_amd")
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream(dev)
    xd, yd = 3, 23
    y = torch.rand(yd, device=dev)
    x = torch.rand(a.rows, xd, device=dev) * 2 - 1
    out = {"rows": a.rows, "steps": a.steps, "device": torch.cuda.get_device_name(0)}
    for W in (256, 512):
        torch.manual_seed(0)
        m = pkg.CDE(xd, yd, [W] * 3)
        ck = os.path.join(ROOT, "tests", "golden", "ckpt_scat.npz")
        if W == 256 and os.path.exists(ck):
            z = np.load(ck)  # keys "<layer>_weight" / "<layer>_bias"; strict: every parameter must be there
            m.sde.a.load_state_dict({k: torch.from_numpy(z[k.replace(".", "_")]) for k in m.sde.a.state_dict()},
                                    strict=True)
        m.sde.a.to(dev)
        flops_col = 2.0 * sum(p.numel() for p in m.sde.a.parameters() if p.ndim == 2)
        cols = 2.0 * a.steps * (1 + xd) * a.rows
        ms, lp = timed(lambda: m.log_prob(x, y, num_steps=a.steps), a.reps, st)
        # the sampler on as many columns: one column-evaluation per chain and step
        chains = a.rows * 2 * (1 + xd)
        ms_s, xs = timed(lambda: m.sample_device(y, chains, a.steps, seed=1, precision="fp32"), a.reps, st)
        out[f"w{W}"] = {
            "weights": "ckpt_scat" if W == 256 and os.path.exists(ck) else "random init",
            "log_prob_ms": ms, "rows_per_s": a.rows / (ms * 1e-3), "ns_per_column_eval": ms * 1e6 / cols,
            "roofline_fraction": cols * flops_col / (ms * 1e-3) / F32_MFMA_PEAK,
            "sampler_f32_ms": ms_s, "sampler_chains": chains, "sampler_ns_per_column_eval": ms_s * 1e6 / (chains * a.steps),
            "sampler_roofline_fraction": chains * a.steps * flops_col / (ms_s * 1e-3) / F32_MFMA_PEAK,
            "finite": bool(torch.isfinite(lp).all() and torch.isfinite(xs).all()),
        }
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
