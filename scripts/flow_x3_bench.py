"""model.log_prob and model.sample_with_log_prob at precision="fp32x3" (csrc/dmip_x3_flow.h) against the exact-f32
kernels they stand beside (csrc/dmip_flow.hip, csrc/dmip_flow_sample.hip), at the reference evaluation's size: 30,000
rows, 200 Heun steps, the scatterometry CDE at [256]^3 (tests/golden/ckpt_scat.npz under the y of
tests/golden/flow_logp.npz case b) and a random [512]^3 under a random y where the fp32x3 kernels are compiled there.
HIP events, fp32 and fp32x3 alternated rep by rep in one session, medians. A density call costs 2 S (1 + xdim) network
column-evaluations per row; the fp32x3 Heun sampler of the same run (2 S per chain, sample_device(solver="heun",
precision="fp32x3")) gives the engine's ns per column-evaluation as the floor. One JSON line, also written to --out
(default profiles/flow_x3/flow_x3_bench.json).
    python scripts/flow_x3_bench.py [--rows 30000] [--steps 200] [--reps 3] [--out PATH]"""
import argparse
import importlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flow_x3", "flow_x3_bench.json"))
    a = ap.parse_args()
    pkg = importlib.import_module("diffusion-modelling-for-inverse-problems_amd")
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream(dev)
    xd, yd = 3, 23
    out = {"rows": a.rows, "steps": a.steps, "reps": a.reps, "device": torch.cuda.get_device_name(0)}
    for W in (256, 512):
        if not pkg._lib.flow_logp_supported(W, 3, xd, yd, precision="fp32x3"):
            out[f"w{W}"] = "no fp32x3 flow kernel compiled at this width"
            continue
        torch.manual_seed(0)
        m = pkg.CDE(xd, yd, [W] * 3)
        ck = os.path.join(ROOT, "tests", "golden", "ckpt_scat.npz")
        fy = os.path.join(ROOT, "tests", "golden", "flow_logp.npz")
        trained = W == 256 and os.path.exists(ck) and os.path.exists(fy)
        if trained:
            z = np.load(ck)  # keys "<layer>_weight" / "<layer>_bias"; strict: every parameter must be there
            m.sde.a.load_state_dict({k: torch.from_numpy(z[k.replace(".", "_")]) for k in m.sde.a.state_dict()},
                                    strict=True)
        m.sde.a.to(dev)
        y = torch.from_numpy(np.load(fy)["b_y"]).to(dev) if trained else torch.rand(yd, device=dev)
        cols = 2.0 * a.steps * (1 + xd) * a.rows  # of either density call
        heun_cols = 2.0 * a.steps * a.rows

        def sample(prec):
            return m.sample_with_log_prob(y, a.rows, a.steps, seed=1, precision=prec)

        def heun():
            return m.sample_device(y, a.rows, a.steps, seed=1, precision="fp32x3", solver="heun")[0]

        x32, q32 = sample("fp32")  # warm-up of every shape the timed window uses; the rows of log_prob
        x3, q3 = sample("fp32x3")
        xh = heun()

        def logp(prec):
            return m.log_prob(x32, y, num_steps=a.steps, precision=prec)

        p32, p3 = logp("fp32"), logp("fp32x3")
        t = {k: [] for k in ("sample_fp32", "sample_fp32x3", "logp_fp32", "logp_fp32x3", "heun_fp32x3")}
        for _ in range(a.reps):  # alternated: other work shares the host
            t["sample_fp32"].append(event_ms(lambda: sample("fp32"), st)[0])
            t["sample_fp32x3"].append(event_ms(lambda: sample("fp32x3"), st)[0])
            t["logp_fp32"].append(event_ms(lambda: logp("fp32"), st)[0])
            t["logp_fp32x3"].append(event_ms(lambda: logp("fp32x3"), st)[0])
            t["heun_fp32x3"].append(event_ms(heun, st)[0])
        med = {k: float(np.median(v)) for k, v in t.items()}
        r = {"weights": "ckpt_scat" if trained else "random init",
             "y": "flow_logp.npz b_y" if trained else "uniform random", "ms_all": t}
        for call in ("sample", "logp"):
            for prec in ("fp32", "fp32x3"):
                ms = med[f"{call}_{prec}"]
                r[f"{call}_{prec}"] = {"ms": ms, "rows_per_s": a.rows / (ms * 1e-3),
                                       "ns_per_column_eval": ms * 1e6 / cols}
            r[f"{call}_fp32_over_fp32x3"] = med[f"{call}_fp32"] / med[f"{call}_fp32x3"]
        r["heun_fp32x3"] = {"ms": med["heun_fp32x3"], "ns_per_column_eval": med["heun_fp32x3"] * 1e6 / heun_cols}
        r["sample_fp32x3_ns_per_eval_over_heun_floor"] = \
            r["sample_fp32x3"]["ns_per_column_eval"] / r["heun_fp32x3"]["ns_per_column_eval"]
        r["x_bitwise_the_fp32x3_heun_sampler"] = bool(torch.equal(x3, xh))
        d = lambda u, v: {"median": float((u - v).abs().median()), "max": float((u - v).abs().max())}  # noqa: E731
        r["logq_fp32x3_vs_fp32_abs_diff"] = d(q3, q32)
        r["logp_fp32x3_vs_fp32_abs_diff"] = d(p3, p32)
        r["finite"] = bool(all(torch.isfinite(v).all() for v in (x32, q32, x3, q3, p32, p3)))
        out[f"w{W}"] = r
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
