"""x3k_bits.npz: the k-major fp32x3 CDE sampler's output bits (csrc/dmip_x3k.h), for tests/test_gpu_x3k_bits.py.

The fixture pins `CDE.sample_device(..., precision="fp32x3")` at hidden_layers [256]*3 bit for bit: a change of the
kernel that only moves or copies values (register classes, staging through LDS, the ring's barriers, instruction
order) must reproduce every entry. It is recorded on an MI355X from the build of the commit BEFORE such a change:

    DMIP_LIB=<that build's libdmip.so> python tests/golden/make_x3k_bits.py [out.npz]   (default: x3k_bits.npz here)

The recorded commit (DMIP_GOLDEN_COMMIT, else the tree's HEAD) and the library's SHA-256 are stored in the file
(`meta`); tests/golden/x3k_bits.md says how the committed file was made. A difference is a bug in the kernel,
never a reason to record again; a new case gets its entry from the code that precedes the change it guards.

The cases and how each one runs live here (`CASES`, `run_case`), so the test and the recording cannot drift apart.
Weights: the scatterometry checkpoint (tests/golden/ckpt_scat.npz) at (xdim, ydim) = (3, 23); at (2, 2) uniform
+-1/sqrt(fan_in) weights from numpy's frozen RandomState stream (no dependence on torch's initialisers).
"""
import hashlib
import importlib
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
PKG = "diffusion-modelling-for-inverse-problems_amd"
PREC = "fp32x3"
S = 17  # no multiple of the ring period (16 chunks per step, 4 slots), nor of the snapshot interval

SHAPES = {"scat": (3, 23), "lin": (2, 2)}


def _cases():
    out = []
    for shp in SHAPES:
        for n in (49, 97):  # a ragged last job (3 x 16 chains) and a partly empty tile
            out.append(dict(id=f"{shp}-n{n}", shape=shp, n=n, S=S, kind="plain"))
            out.append(dict(id=f"{shp}-n{n}-2y", shape=shp, n=n, S=S, kind="two_y"))
            out.append(dict(id=f"{shp}-n{n}-shards", shape=shp, n=n, S=S, kind="shards"))
            out.append(dict(id=f"{shp}-n{n}-snaps", shape=shp, n=n, S=S, kind="snaps", every=4))
        for nt in ("1", "2"):  # the 8-wave form (NT = 1) has other piece and barrier counts
            out.append(dict(id=f"{shp}-n97-nt{nt}", shape=shp, n=97, S=S, kind="plain", nt=nt))
    # more jobs (1,025 of 48 chains) than the 1,024 resident waves: segment kinds 1, 2 and 3 (hand-over) all occur
    out.append(dict(id="scat-handover", shape="scat", n=49200, S=5, kind="handover", stride=97))
    return out


CASES = _cases()


def model_and_y(pkg, shape, dev):
    """The network of `shape` on `dev` and two observations (the one-observation cases take the first)."""
    import torch
    xd, yd = SHAPES[shape]
    m = pkg.CDE(xd, yd, [256] * 3)
    lin = [l for l in m.sde.a if isinstance(l, torch.nn.Linear)]
    if shape == "scat":
        z = np.load(os.path.join(HERE, "ckpt_scat.npz"))
        m.sde.a.load_state_dict({k.replace("_", "."): torch.from_numpy(z[k]) for k in z.files
                                 if k.split("_")[0].isdigit()})
        y0 = np.load(os.path.join(HERE, "samples_scat.npz"))["y"].astype(np.float32)
    else:
        rs = np.random.RandomState(20260)
        with torch.no_grad():
            for l in lin:
                b = 1.0 / np.sqrt(l.in_features)
                l.weight.copy_(torch.from_numpy(rs.uniform(-b, b, tuple(l.weight.shape)).astype(np.float32)))
                l.bias.copy_(torch.from_numpy(rs.uniform(-b, b, tuple(l.bias.shape)).astype(np.float32)))
        y0 = np.array([0.5, 1.0], np.float32)
    y1 = (y0 + np.random.RandomState(7).uniform(-0.25, 0.25, y0.shape)).astype(np.float32)
    return m, torch.from_numpy(np.stack([y0, y1])).to(dev)


def run_case(pkg, models, c, dev="cuda:0"):
    """name -> array of what case `c` stores or compares. DMIP_X3K_NT is read at every launch."""
    if c["shape"] not in models:
        models[c["shape"]] = model_and_y(pkg, c["shape"], dev)
    m, ys = models[c["shape"]]
    n, steps, seed = c["n"], c["S"], 1000 + c["n"]
    os.environ["DMIP_X3P"] = "0"  # the k-major engine under the A/B library too
    old_nt = os.environ.get("DMIP_X3K_NT")
    os.environ["DMIP_X3K_NT"] = c.get("nt", "3")
    try:
        if c["kind"] == "two_y":
            return {"x": m.sample_device(ys, n, steps, seed=seed, precision=PREC).cpu().numpy()}
        if c["kind"] == "shards":  # two halves are the whole: stored as the whole
            h = n // 2
            a = m.sample_device(ys[0], h, steps, seed=seed, chain_offset=0, precision=PREC)
            b = m.sample_device(ys[0], n - h, steps, seed=seed, chain_offset=h, precision=PREC)
            return {"x": np.concatenate([a.cpu().numpy(), b.cpu().numpy()], axis=1)}
        if c["kind"] == "snaps":
            x, snaps = m.sample_trajectory(ys[0], n, steps, c["every"], seed=seed, precision=PREC)
            return {"x": x.cpu().numpy(), "snaps": snaps.cpu().numpy()}
        x = m.sample_device(ys[0], n, steps, seed=seed, precision=PREC).cpu().numpy()
        pkg._lib.device_status(dev)
        if c["kind"] == "handover":
            sha = np.frombuffer(hashlib.sha256(np.ascontiguousarray(x).tobytes()).digest(), np.uint8)
            return {"x": np.ascontiguousarray(x[:, ::c["stride"]]), "sha256": sha}
        return {"x": x}
    finally:
        if old_nt is None:
            os.environ.pop("DMIP_X3K_NT", None)
        else:
            os.environ["DMIP_X3K_NT"] = old_nt


def main():
    import torch
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "x3k_bits.npz")
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    pkg = importlib.import_module(PKG)
    assert torch.cuda.is_available(), "recording needs an MI355X"
    models, arrays = {}, {}
    for c in CASES:
        for k, v in run_case(pkg, models, c).items():
            assert v.dtype == np.uint8 or np.all(np.isfinite(v)), c["id"]
            arrays[f"{c['id']}/{k}"] = v
    # shards of the recording build agree with its whole run (else the fixture would pin a sharding bug)
    for shp in SHAPES:
        for n in (49, 97):
            assert np.array_equal(arrays[f"{shp}-n{n}/x"], arrays[f"{shp}-n{n}-shards/x"]), (shp, n)
            assert np.array_equal(arrays[f"{shp}-n{n}/x"], arrays[f"{shp}-n{n}-snaps/x"]), (shp, n)
    lib = pkg._lib.LIB_PATH
    try:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip()
    except OSError:
        commit = ""
    meta = {"library_sha256": hashlib.sha256(open(lib, "rb").read()).hexdigest(),
            "commit": os.environ.get("DMIP_GOLDEN_COMMIT", commit), "device": torch.cuda.get_device_name(0)}
    arrays["meta"] = np.frombuffer(json.dumps(meta).encode(), np.uint8)
    np.savez_compressed(out, **arrays)
    print(json.dumps({"out": out, "entries": len(arrays), "bytes": os.path.getsize(out), **meta}), flush=True)


if __name__ == "__main__":
    main()
