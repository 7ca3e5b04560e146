"""LinearDPS with guidance='tweedie' (csrc/dmip_dps_tweedie.hip, csrc/dmip_x3_dps_tweedie.hip) beside guidance='pigdm'
(csrc/dmip_dps_linear.hip, csrc/dmip_x3_dps_linear.hip) on the same prior, problem and shape: 100,000 chains x 200 steps
at [64]^3 / xdim 2 (the linear problem's A, b, Sigma; ydim 2) and at [512]^3 / xdim 3 (a random 23 x 3 operator), exact
f32 and fp32x3, HIP events, the calls alternated rep by rep in one session, medians. The two differ by one D x D solve
per chain and step; the figure is the ratio tweedie / pigdm. Random initial weights at the default SDE; zeta = 1e-4 for
both keeps pigdm's chains finite on an untrained prior, so both time the same finite arithmetic. One
JSON line, also written to --out (default profiles/dps_tweedie/dps_tweedie_bench.json).
    python scripts/dps_tweedie_bench.py [--chains 100000] [--steps 200] [--reps 3] [--out PATH]"""
import argparse
import importlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GUIDANCES = ("tweedie", "pigdm")


def event_ms(fn, st):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    out = fn()
    e1.record(st)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=100000)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dps_tweedie", "dps_tweedie_bench.json"))
    a = ap.parse_args()
    pkg = importlib.import_module("diffusion-modelling-for-inverse-problems_amd")
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream(dev)
    out = {"chains": a.chains, "steps": a.steps, "reps": a.reps, "zeta": 1e-4,
           "device": torch.cuda.get_device_name(0)}
    prob = pkg.LinearForwardProblem()
    rng = np.random.default_rng(0)
    for W, xd, yd in ((64, 2, 2), (512, 3, 23)):
        if xd == 2:
            A, b, Sigma = prob.A.numpy(), prob.b.numpy(), prob.Sigma.numpy()
        else:
            A, b, Sigma = rng.normal(size=(yd, xd)) / np.sqrt(xd), rng.normal(size=yd), 0.3
        models = {}
        for g in GUIDANCES:
            torch.manual_seed(0)  # the same weights
            models[g] = pkg.LinearDPS(xd, yd, [W] * 3, A, b, Sigma, zeta=1e-4, guidance=g)
            models[g].sde.a.to(dev)
        y = torch.rand(yd, device=dev)
        calls = {f"{g}_{prec}": (lambda g=g, p=prec: models[g].sample_device(y, a.chains, a.steps, seed=1, precision=p))
                 for prec in ("fp32", "fp32x3") for g in GUIDANCES}
        outs = {k: fn() for k, fn in calls.items()}  # warm-up of everything the timed window uses (tables included)
        t = {k: [] for k in calls}
        for _ in range(a.reps):  # alternated: other work shares the host
            for k, fn in calls.items():
                t[k].append(event_ms(fn, st)[0])
        pkg._lib.clear_range_status(dev)
        r = {"ms_all": t}
        for k in calls:
            ms = float(np.median(t[k]))
            r[k] = {"ms": ms, "chains_per_s": a.chains / (ms * 1e-3), "finite": bool(torch.isfinite(outs[k]).all())}
        for prec in ("fp32", "fp32x3"):
            r[f"tweedie_over_pigdm_{prec}"] = r[f"tweedie_{prec}"]["ms"] / r[f"pigdm_{prec}"]["ms"]
            r[f"pigdm_spread_{prec}"] = max(t[f"pigdm_{prec}"]) / min(t[f"pigdm_{prec}"])
        out[f"w{W}_x{xd}_y{yd}"] = r
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
