"""Timings of the paired flow kernels (model.log_prob_pairs) against the per-y route, HIP events, median of 3, the two
calls alternated in one process (results in profiles/pairs/):
  pairs_vs_per_y   log_prob_pairs(x, ys) against log_prob(x[:, None, :], ys), n pairs with a different y each
  bias_loads       log_prob_pairs with every row sharing one y against log_prob(x, y): the cost of the per-row bias
at [64]^3 xdim 2 / ydim 2 and [512]^3 xdim 3 / ydim 23, precision fp32 and fp32x3, 200 steps.
    python scripts/pairs_bench.py --out profiles/pairs/pairs_bench.json [--pairs 10000 --rows 30000 --steps 200]
"""
import argparse
import importlib
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
dmip = importlib.import_module("diffusion-modelling-for-inverse-problems_amd")
DEV = "cuda:0"
SHAPES = {"w64": (64, 2, 2), "w512": (512, 3, 23)}


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def alternate(f, g, reps=3):
    f(), g()  # warm-up: handles, images, code objects
    torch.cuda.synchronize()
    tf, tg = [], []
    for _ in range(reps):
        tf.append(timed(f)[0])
        tg.append(timed(g)[0])
    return tf, tg


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--pairs", type=int, default=10000)
    ap.add_argument("--rows", type=int, default=30000)
    ap.add_argument("--steps", type=int, default=200)
    args = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "steps": args.steps, "pairs": args.pairs, "rows": args.rows,
           "timer": "HIP events around one call, median of 3, calls alternated", "pairs_vs_per_y": {}, "bias_loads": {}}
    for name, (W, xd, yd) in SHAPES.items():
        torch.manual_seed(W)
        m = dmip.CDE(xd, yd, [W] * 3)
        g = torch.Generator().manual_seed(W + 1)
        for prec in ("fp32", "fp32x3"):
            n = args.pairs
            x = torch.randn(n, xd, generator=g).to(DEV)
            ys = torch.randn(n, yd, generator=g).to(DEV)
            x3 = x[:, None, :].contiguous()
            tp, ty = alternate(lambda: m.log_prob_pairs(x, ys, num_steps=args.steps, precision=prec),
                               lambda: m.log_prob(x3, ys, num_steps=args.steps, precision=prec))
            a = m.log_prob_pairs(x, ys, num_steps=args.steps, precision=prec)
            b = m.log_prob(x3, ys, num_steps=args.steps, precision=prec)[:, 0]
            mp, my = statistics.median(tp), statistics.median(ty)
            res["pairs_vs_per_y"][f"{name}_{prec}"] = {
                "pairs_ms": tp, "per_y_ms": ty, "pairs_median_ms": mp, "per_y_median_ms": my, "speedup": my / mp,
                "max_abs_diff": (a - b).abs().max().item(), "bitwise_equal_rows": int((a == b).sum().item())}
            print(name, prec, "pairs vs per-y", res["pairs_vs_per_y"][f"{name}_{prec}"], flush=True)
            n = args.rows
            x = torch.randn(n, xd, generator=g).to(DEV)
            y1 = torch.randn(yd, generator=g).to(DEV)
            yr = y1[None].expand(n, yd).contiguous()
            tp, ty = alternate(lambda: m.log_prob_pairs(x, yr, num_steps=args.steps, precision=prec),
                               lambda: m.log_prob(x, y1, num_steps=args.steps, precision=prec))
            mp, my = statistics.median(tp), statistics.median(ty)
            res["bias_loads"][f"{name}_{prec}"] = {"pairs_ms": tp, "per_y_ms": ty, "pairs_median_ms": mp,
                                                   "per_y_median_ms": my, "pairs_over_per_y": mp / my}
            print(name, prec, "bias loads", res["bias_loads"][f"{name}_{prec}"], flush=True)
    line = json.dumps(res, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
