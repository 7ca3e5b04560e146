"""Generate tests/golden/mala_io.npz: the REFERENCE's anneal_to_energy with Langevin proposals (langevin_prop=True,
models/SNF.py:250-300) on its own surrogate, with the torch draws it consumed captured beside its results.

Like make_golden.py this runs only where the reference is checked out, touches it only through
make_golden.import_reference(), and writes data only. The draws are recorded the way gen_surrogate records the
random-walk ones (mh_*): seed, draw what the reference will draw -- per Metropolis step lang_steps x randn(n, 3) (the
Langevin noises of langevin_step) and then rand(n) (the acceptance uniform) -- reseed, and run the reference.

All cases: y = y_test[0] of data_scat.npz, 256 chains x 50 steps, x0 = rand(256, 3, Generator(31)) * 2 - 1, draws
under torch.manual_seed(77).
  A  lang_steps 1, stepsize 1e-3, the posterior energy
  B  lang_steps 3, stepsize 2e-4, the posterior energy
  C  lang_steps 1, stepsize 2e-3, get_interpolated_energy_fun(y, 0.5, .)
For every case the script prints the acceptance rate and the share of chains on which the float64 restatement of the
scheme (tests/mala_ref.py) fed the same draws ends within 1e-5 of the reference's float32 run: the ceiling of any path
test on this fixture (a borderline acceptance flips on a last-bit energy difference).

Usage:  python tests/golden/make_golden_mala.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))            # tests/: mala_ref
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))  # the repository root: oracle
import make_golden as MG  # noqa: E402

CASES = {"A": (1, 1e-3, 1.0), "B": (3, 2e-4, 1.0), "C": (1, 2e-3, 0.5)}
N, S, X0_SEED, DRAW_SEED = 256, 50, 31, 77


def main():
    R = MG.import_reference()
    import torch
    import mala_ref
    import oracle as O
    torch.set_num_threads(os.cpu_count())
    fm, prm = R.scat.load_forward_model(os.path.join(MG.REF, "trained_models/scatterometry"))
    a, b, lam = prm["a"], prm["b"], prm["lambd_bd"]
    y0 = torch.from_numpy(np.load(os.path.join(HERE, "data_scat.npz"))["y_test"][0])
    params = O.surrogate_params_from_npz(np.load(os.path.join(HERE, "surrogate.npz")))
    x0 = torch.rand(N, 3, generator=torch.Generator().manual_seed(X0_SEED)) * 2 - 1
    out = {"y": y0.numpy(), "x0": x0.numpy(), "a": a, "b": b, "lambd_bd": lam, "draw_seed": DRAW_SEED}
    for tag, (L, h, lambd) in CASES.items():
        post = lambda v, ys: R.scat.get_log_posterior(v, fm, a, b, ys, lam)
        en = R.snf.get_interpolated_energy_fun(y0[None, :].repeat(N, 1), lambd, post)
        torch.manual_seed(DRAW_SEED)
        eta, u = [], []
        for _ in range(S):
            eta.append(torch.stack([torch.randn(N, 3) for _ in range(L)]))
            u.append(torch.rand(N))
        eta, u = torch.stack(eta).numpy(), torch.stack(u).numpy()
        torch.manual_seed(DRAW_SEED)
        xs, ediff = R.snf.anneal_to_energy(x0.clone(), en, S, langevin_prop=True, lang_steps=L, stepsize=h)
        xs, ediff = xs.detach().numpy(), ediff.detach().numpy()
        xr, _, nacc = mala_ref.mala_sample(params, y0.numpy(), S, h, L, lambd, a, b, lam, x0=x0.numpy(), eta=eta, unif=u)
        d = np.abs(xs - xr).max(1)
        share = float(np.mean(d <= 1e-5))
        print(f"case {tag}: lang_steps {L} stepsize {h:g} lambd {lambd:g}: acceptance {nacc.mean() / S:.3f}, on the "
              f"reference's path (max |dx| <= 1e-5, f32 reference vs f64 restatement) {share:.3f}, median |dx| "
              f"{np.median(d):.1e}, finite {bool(np.isfinite(xs).all())}")
        out.update({f"{tag}_lang_steps": L, f"{tag}_stepsize": h, f"{tag}_lambd": lambd, f"{tag}_eta": eta,
                    f"{tag}_u": u, f"{tag}_x": xs, f"{tag}_ediff": ediff, f"{tag}_path_share": share,
                    f"{tag}_accept": float(nacc.mean() / S)})
    np.savez(os.path.join(HERE, "mala_io.npz"), **out)


if __name__ == "__main__":
    main()
