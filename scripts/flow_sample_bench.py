"""model.sample_with_log_prob (csrc/dmip_flow_sample.hip) against what it replaces -- sample_device(solver="heun",
precision="fp32") followed by log_prob on the result -- at the reference evaluation's size: 30,000 rows, 200 Heun
steps, the scatterometry CDE at [256]^3 (tests/golden/ckpt_scat.npz, under the y of tests/golden/flow_logp.npz case
b) and at the reference width [512]^3 (random init, random y;
the exact-f32 Heun sampler has no fused kernel at that width, so its two-call path samples through the per-step
loop: "heun_path"). HIP events, the two paths alternated rep by rep in one session, medians. The fused launch and
log_prob both cost 2 S (1 + xdim) network column-evaluations per row, the Heun sampler 2 S more; the roofline
fraction counts 2 * weights flops per column-evaluation against the f32 MFMA peak. One JSON line, also written to
--out (default profiles/flow_sample/flow_sample_bench.json).
    python scripts/flow_sample_bench.py [--rows 30000] [--steps 200] [--reps 3] [--out PATH]"""
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


def event_ms(fn, st):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    out = fn()
    e1.record(st)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=30000)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flow_sample", "flow_sample_bench.json"))
    a = ap.parse_args()
    pkg = importlib.import_module("diffusion-modelling-for-inverse-problems_amd")
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream(dev)
    xd, yd = 3, 23
    y_rand = torch.rand(yd, device=dev)
    out = {"rows": a.rows, "steps": a.steps, "reps": a.reps, "device": torch.cuda.get_device_name(0)}
    for W in (256, 512):
        torch.manual_seed(0)
        m = pkg.CDE(xd, yd, [W] * 3)
        ck = os.path.join(ROOT, "tests", "golden", "ckpt_scat.npz")
        if W == 256 and os.path.exists(ck):
            z = np.load(ck)  # keys "<layer>_weight" / "<layer>_bias"; strict: every parameter must be there
            m.sde.a.load_state_dict({k: torch.from_numpy(z[k.replace(".", "_")]) for k in m.sde.a.state_dict()},
                                    strict=True)
        m.sde.a.to(dev)
        # the trained checkpoint under an observation of its own problem (the log-likelihood fixture's): under a
        # random y its chains leave the training box and neither discretisation of the density has converged
        fy = os.path.join(ROOT, "tests", "golden", "flow_logp.npz")
        trained_y = W == 256 and os.path.exists(ck) and os.path.exists(fy)
        y = torch.from_numpy(np.load(fy)["b_y"]).to(dev) if trained_y else y_rand
        flops_col = 2.0 * sum(p.numel() for p in m.sde.a.parameters() if p.ndim == 2)
        cols = 2.0 * a.steps * (1 + xd) * a.rows  # of the fused launch, and of log_prob alone

        def fused():
            return m.sample_with_log_prob(y, a.rows, a.steps, seed=1)

        def sample():
            return m.sample_device(y, a.rows, a.steps, seed=1, precision="fp32", solver="heun")[0]

        calls0 = dict(pkg._lib.calls)
        x_f, lq_f = fused()  # warm-up of every shape the timed window uses
        x_s = sample()
        lp = m.log_prob(x_s, y, num_steps=a.steps)
        heun_fused = pkg._lib.calls.get("ode_sample", 0) > calls0.get("ode_sample", 0)
        t_f, t_s, t_l = [], [], []
        for _ in range(a.reps):  # alternated: other work shares the host
            t_f.append(event_ms(fused, st)[0])
            ms, xs = event_ms(sample, st)
            t_s.append(ms)
            t_l.append(event_ms(lambda: m.log_prob(xs, y, num_steps=a.steps), st)[0])
        f_ms, s_ms, l_ms = (float(np.median(t)) for t in (t_f, t_s, t_l))
        two_ms = float(np.median([s + l for s, l in zip(t_s, t_l)]))
        out[f"w{W}"] = {
            "weights": "ckpt_scat" if W == 256 and os.path.exists(ck) else "random init",
            "y": "flow_logp.npz b_y" if trained_y else "uniform random",
            "fused_ms": f_ms, "fused_ms_all": t_f, "fused_rows_per_s": a.rows / (f_ms * 1e-3),
            "fused_ns_per_column_eval": f_ms * 1e6 / cols,
            "fused_roofline_fraction": cols * flops_col / (f_ms * 1e-3) / F32_MFMA_PEAK,
            "heun_path": "fused (dmip_ode_sample)" if heun_fused else "per-step loop (no exact-f32 Heun kernel)",
            "heun_sample_ms": s_ms, "log_prob_ms": l_ms, "log_prob_ns_per_column_eval": l_ms * 1e6 / cols,
            "two_call_ms": two_ms, "two_call_over_fused": two_ms / f_ms,
            # same seed, same steps: the fused x is the sampler's x where that ran the fused Heun kernel
            "x_max_abs_diff_vs_sampler": float((x_f - x_s).abs().max()),
            # the two Heun grids of one integral at this step count (meaningful for the trained checkpoint under its
            # own y; untrained weights grow |x| without bound and the difference with them)
            "logq_vs_log_prob_abs_diff": {"median": float((lq_f - lp).abs().median()),
                                          "p99": float((lq_f - lp).abs().double().quantile(0.99)),
                                          "max": float((lq_f - lp).abs().max())},
            "finite": bool(torch.isfinite(lq_f).all() and torch.isfinite(x_f).all() and torch.isfinite(lp).all()),
        }
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
