"""Evaluation drivers with the reference's signatures and metrics:
`evaluate_scatterometry` = main_diffusion_scatterometry.py:40-124 `evaluate`, `evaluate_linear` =
main_diffusion_linear.py:53-137 `evaluate`.

Same metrics and `results.csv` columns as the reference (KL2 / KL_reverse from 75-bin histograms with
epsilon smoothing and `rel_entr`, NLL, score MSE at t = 0), computed on the device:
  * all `n_repeats` draws of one y are one fused-sampler launch (`sample_device` with the y row
    repeated: repeat j is y-row j, its own RNG stream), instead of n_repeats host round trips;
  * histograms are `dmip_histogram` (numpy.histogramdd-exact binning, csrc/dmip_eval.hip), KL in
    float64 on the device.
Under torch.distributed (world_size > 1) the ys are sharded over the ranks (parallel.map_sharded:
each rank samples and scores its contiguous range of ys; one all_gather of the per-y metric rows;
rank 0 writes results.csv). Deliberate difference: the reference returns `mse_score_vals.mean()` on a Python list
(AttributeError at :124 / :137); here the mean is taken.
"""
import os

import numpy as np
import torch

from . import _lib, parallel
from .problems import get_gt_samples_scatterometry, get_log_posterior


def histograms(samples, nbins, xlim):
    """(n_hist, n, d) samples -> (n_hist, nbins**d) int32 counts, numpy.histogramdd binning."""
    x = samples.to(dtype=torch.float32).contiguous()
    if x.ndim == 2:
        x = x[None]
    counts = torch.zeros(x.shape[0], nbins ** x.shape[2], dtype=torch.int32, device=x.device)
    _lib.histogram(x, nbins, xlim[0], xlim[1], counts)
    return counts


def hist_kl(counts_true, counts_model, epsilon=1e-10):
    """KL2 and reverse KL of two count histograms exactly as the reference drivers compute them
    (normalise, + epsilon, renormalise, sum rel_entr) -- float64 on the device."""
    p = counts_true.to(torch.float64)
    q = counts_model.to(torch.float64)
    p = p / p.sum()
    q = q / q.sum()
    p = p + epsilon
    q = q + epsilon
    p = p / p.sum()
    q = q / q.sum()
    kl = torch.sum(p * torch.log(p / q))
    klr = torch.sum(q * torch.log(q / p))
    return float(kl), float(klr)


def _is_root():
    return parallel.world()[0] == 0


def _write_results(out_dir, columns):
    import pandas as pd
    if out_dir:
        os.makedirs(out_dir, exist_ok=True)
        pd.DataFrame(columns).to_csv(os.path.join(out_dir, 'results.csv'))


def _plot(x, nbins, xlim, fname, **kw):
    try:
        from .refapi.utils import plot_density
    except Exception:  # plotting is optional (matplotlib)
        return
    plot_density(x, nbins, limits=xlim, fname=fname, **kw)


def evaluate_scatterometry(model, ys, forward_model, out_dir, plot_ys, n_samples_x, score_posterior, a, b,
                           lambd_bd, gt_dir, n_repeats=10, epsilon=1e-10, xlim=(-1.2, 1.2), nbins=75,
                           figsize=(12, 12), labelsize=30, gt_loader=None, num_steps=200):
    """main_diffusion_scatterometry.py:40-124. `gt_loader(i, j)` overrides the MCMC ground-truth
    files (`gt_dir/<i>/<j>.npy`, generate_scatterometry_ground_truth.py)."""
    dev = model._exec_device(ys)
    ys = torch.as_tensor(ys).to(device=dev, dtype=torch.float32)
    load = gt_loader or (lambda i, j: get_gt_samples_scatterometry(gt_dir, i, j))

    def one_y(i):
        y = ys[i]
        # (R, N, 3); the default precision's fp16-range guard (parallel.sample_checked) -- this rank's own y
        x_pred = parallel.sample_checked(model, y.expand(n_repeats, -1), n_samples_x, num_steps, 0, 1)
        x_true = torch.stack([torch.as_tensor(load(i, j)).to(device=dev, dtype=torch.float32)
                              for j in range(n_repeats)])
        inflated = y[None, :].expand(x_true.shape[1], -1)
        nll_t = nll_d = mse = 0.0
        for j in range(n_repeats):
            xt = x_true[j]
            t0 = torch.zeros(xt.shape[0], 1, device=dev)
            with torch.no_grad():
                s_pred = model.sde.a(xt, inflated, t0) / model.sde.base_sde.g(t0, xt)
            s_true = score_posterior(xt, inflated)
            mse += float(torch.mean(torch.sum((s_pred - s_true) ** 2, dim=1)))
            with torch.no_grad():
                nll_t += float(get_log_posterior(xt, forward_model, a, b, inflated, lambd_bd).sum()) / n_samples_x
                nll_d += float(get_log_posterior(x_pred[j], forward_model, a, b,
                                                 y[None, :].expand(x_pred.shape[1], -1), lambd_bd).sum()) / n_samples_x
        ht = histograms(x_true.reshape(1, -1, 3), nbins, xlim)[0]
        hd = histograms(x_pred.reshape(1, -1, 3), nbins, xlim)[0]
        kl, klr = hist_kl(ht, hd, epsilon)
        if i in plot_ys and out_dir:
            _plot(x_true[-1].cpu().numpy(), nbins, xlim, os.path.join(out_dir, 'posterior-mcmc-%d.svg' % i),
                  xticks=[-1, 0, 1], size=figsize, labelsize=labelsize)
            _plot(x_pred[-1].cpu().numpy(), nbins, xlim, os.path.join(out_dir, 'posterior-diffusion-%d.svg' % i),
                  xticks=[-1, 0, 1], size=figsize, labelsize=labelsize)
        return kl, klr, nll_t / n_repeats, nll_d / n_repeats, mse / n_repeats

    kl2_vals, kl2_rev, nll_mcmc, nll_diff, mse_vals = parallel.map_sharded(ys.shape[0], one_y, 5).T
    nlpd = np.abs(nll_diff - nll_mcmc)
    if _is_root():
        _write_results(out_dir, {'KL2': kl2_vals, 'KL_reverse': kl2_rev, 'NLL_mcmc': nll_mcmc,
                                 'NLL_diffusion': nll_diff, 'MSE': mse_vals})
        print('KL2:', kl2_vals.mean(), '+-', np.mean((kl2_vals - kl2_vals.mean()) ** 2))
    return kl2_vals.mean(), nlpd.mean(), float(np.mean(mse_vals))


def evaluate_linear(model, ys, forward_model, out_dir, plot_ys, n_samples_x=5000, n_repeats=10, epsilon=1e-10,
                    xlim=(-3.5, 3.5), nbins=75, figsize=(12, 12), labelsize=30, num_steps=200):
    """main_diffusion_linear.py:53-137, against the analytic Gaussian posterior."""
    dev = model._exec_device(ys)
    ys = torch.as_tensor(ys).to(device=dev, dtype=torch.float32)
    model.sde.eval()

    def one_y(i):
        y = ys[i]
        posterior = forward_model.get_posterior(y.cpu(), device='cpu')
        x_pred = parallel.sample_checked(model, y.expand(n_repeats, -1), n_samples_x, num_steps, 0, 1)  # (R, N, 2)
        x_true = posterior.sample((n_repeats, n_samples_x)).to(device=dev, dtype=torch.float32)
        nll_t = nll_d = mse = 0.0
        for j in range(n_repeats):
            xt = x_true[j]
            t0 = torch.zeros(xt.shape[0], 1, device=dev)
            inflated = torch.ones_like(xt) * y
            with torch.no_grad():
                s_pred = model.sde.a(xt, inflated, t0) / model.sde.base_sde.g(t0, xt)
            s_true = forward_model.score_posterior(xt, inflated)
            mse += float(torch.mean(torch.sum((s_pred - s_true) ** 2, dim=1)))
            nll_t -= float(torch.mean(posterior.log_prob(xt.cpu())))
            nll_d -= float(torch.mean(posterior.log_prob(x_pred[j].cpu())))
        ht = histograms(x_true.reshape(1, -1, 2), nbins, xlim)[0]
        hd = histograms(x_pred.reshape(1, -1, 2), nbins, xlim)[0]
        kl, _ = hist_kl(ht, hd, epsilon)
        if i in plot_ys and out_dir:
            _plot(x_true[-1].cpu().numpy(), nbins, xlim, os.path.join(out_dir, 'posterior-true-%d.svg' % i),
                  xticks=xlim, size=figsize, labelsize=labelsize, show_mean=True)
            _plot(x_pred[-1].cpu().numpy(), nbins, xlim, os.path.join(out_dir, 'posterior-diffusion-%d.svg' % i),
                  xticks=xlim, size=figsize, labelsize=labelsize, show_mean=True)
        return kl, nll_t / n_repeats, nll_d / n_repeats, mse / n_repeats

    kl2_vals, nll_true, nll_diff, mse_vals = parallel.map_sharded(ys.shape[0], one_y, 4).T
    nlpd = np.abs(nll_true - nll_diff)
    if _is_root():
        _write_results(out_dir, {'KL2': kl2_vals, 'NLL_true': nll_true, 'NLL_diffusion': nll_diff,
                                 'MSE': mse_vals})
        print('KL2:', kl2_vals.mean(), '+-', np.mean((kl2_vals - kl2_vals.mean()) ** 2))
    return kl2_vals.mean(), nlpd.mean(), float(np.mean(mse_vals))


# --------------------------------------------------------------------------- importance sampling with log q
def _f64(v):
    v = v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
    return np.asarray(v, np.float64)


def importance_report(logq, log_target):
    """What samples x ~ q with their density say about an unnormalised target: `logq` = log q(x) (e.g. of
    model.sample_with_log_prob) and `log_target` = the unnormalised log posterior at the same samples, both (n,) or
    (n_y, n), tensors or arrays. Float64 on the host; every exponential is taken of log weights shifted by their
    row maximum, so no shift of either argument overflows. Returns a dict, per row of (n_y, n) inputs ((n,) inputs:
    scalars, weights (n,)):
        ess         (sum w)^2 / sum w^2 of w = target / q: the effective sample size, in [1, n]
        ess_frac    ess / n
        log_z       log mean w: the log evidence of the target under q (log of its normalising constant)
        reverse_kl  mean(logq - log_target) + log_z: the Monte-Carlo KL(q || target / Z) with the estimated Z
        weights     w / sum w
    """
    lq, lt = _f64(logq), _f64(log_target)
    if lq.shape != lt.shape or lq.ndim not in (1, 2) or lq.shape[-1] < 1:
        raise ValueError("importance_report: logq and log_target must both be (n,) or (n_y, n)")
    lw = lt - lq
    n = lw.shape[-1]
    mx = lw.max(axis=-1, keepdims=True)
    w = np.exp(lw - mx)
    s1, s2 = w.sum(axis=-1), (w * w).sum(axis=-1)
    ess = s1 * s1 / s2
    log_z = np.log(s1 / n) + mx[..., 0]
    # mean(-lw) + log_z with the shift taken out first: exact 0 for target == q whatever the common offset
    reverse_kl = np.log(s1 / n) - (lw - mx).mean(axis=-1)
    out = {"ess": ess, "ess_frac": ess / n, "log_z": log_z, "reverse_kl": reverse_kl, "weights": w / s1[..., None]}
    return {k: (float(v) if np.ndim(v) == 0 else v) for k, v in out.items()}


def importance_posterior(model, y, log_target_fn, num_samples=4096, num_steps=200, seed=None, precision=None):
    """Self-checking posterior samples for one observation y (ydim,): model.sample_with_log_prob, then
    importance_report against `log_target_fn(x)` -> (n,), the unnormalised log posterior at the device samples
    x (n, xdim). Targets of the two problems of this package:
        linear          post = LinearForwardProblem().get_posterior(y.cpu(), device='cpu')
                        lambda x: post.log_prob(x.cpu())      (the drivers' way: the 2 x 2 Gaussian on the host)
        scatterometry   lambda x: -get_log_posterior(x, forward_model, a, b, y, lambd_bd)
                        (get_log_posterior returns the negative log posterior, (n, 1) or (n,): it is flattened)
    Returns importance_report's dict plus x (n, xdim) and logq (n,) (device tensors) and, in float64 numpy,
    mean (the plain sample mean of x), snis_mean and snis_cov (the self-normalised importance-sampling mean and
    covariance: sum_i w_i x_i and sum_i w_i (x_i - m)(x_i - m)^T with the normalised weights). `precision` is
    sample_with_log_prob's (None: exact f32; "fp32x3": the split-fp16 engine)."""
    x, logq = model.sample_with_log_prob(torch.as_tensor(y).reshape(-1), num_samples, num_steps, seed=seed,
                                         precision=precision)
    lt = torch.as_tensor(log_target_fn(x)).reshape(-1)
    rep = importance_report(logq, lt)
    xs, w = _f64(x), rep["weights"]
    m = w @ xs
    r = xs - m
    rep.update(x=x, logq=logq, mean=xs.mean(axis=0), snis_mean=m, snis_cov=(w[:, None] * r).T @ r)
    return rep


# --------------------------------------------------------------------------- paired workloads: one observation per row
DEFAULT_LEVELS = tuple(i / 20 for i in range(1, 20))  # credibility levels 0.05 .. 0.95


def held_out_log_prob(model, x, y, num_steps=200, precision=None):
    """Held-out conditional negative log-likelihood of a test set of pairs, x (n, xdim) and y (n, ydim): the
    model-selection number that needs no MCMC ground truth. One model.log_prob_pairs call; the sums in float64 on the
    host. Returns {"nll": -mean log p(x_i | y_i), "stderr": its standard error (the sample standard deviation, n - 1,
    over sqrt(n); 0.0 for n = 1), "n": n}."""
    lp = _f64(model.log_prob_pairs(x, y, num_steps=num_steps, precision=precision)).reshape(-1)
    n = lp.shape[0]
    mean = lp.sum() / n
    var = ((lp - mean) ** 2).sum() / (n - 1) if n > 1 else 0.0
    return {"nll": float(-mean), "stderr": float(np.sqrt(var / n)), "n": int(n)}


def coverage_from_logq(logq_truth, logq_samples, levels=DEFAULT_LEVELS):
    """Expected coverage of highest-posterior-density regions from log-densities alone (a pure host function, float64).
    logq_truth (n,): log q(x_true_i | y_i); logq_samples (n, L): log q of L samples of q(. | y_i). alpha_i is the
    fraction of row i's samples whose log q exceeds the truth's: the credibility level of the smallest HPD region of
    q(. | y_i) that holds x_true_i. The expected coverage at a level is mean(alpha_i <= level); for a calibrated q,
    alpha is uniform on (0, 1) and coverage equals level. Returns {"alpha": (n,), "levels": (k,), "coverage": (k,)}."""
    lt, ls = _f64(logq_truth).reshape(-1), _f64(logq_samples)
    if ls.ndim != 2 or ls.shape[0] != lt.shape[0] or ls.shape[1] < 1:
        raise ValueError("coverage_from_logq: logq_truth must be (n,) and logq_samples (n, L)")
    lv = np.asarray(levels, np.float64).reshape(-1)
    alpha = (ls > lt[:, None]).sum(axis=1) / ls.shape[1]
    return {"alpha": alpha, "levels": lv, "coverage": (alpha[:, None] <= lv[None, :]).mean(axis=0)}


def hpd_coverage(model, x_true, y, num_samples, num_steps=200, levels=DEFAULT_LEVELS, seed=None, precision=None):
    """Calibration of an amortised estimator over simulated pairs x_true (n, xdim), y (n, ydim): num_samples draws of
    q(. | y_i) with their log q per observation (model.sample_with_log_prob, the multi-y path: many rows per y is what
    it is built for), log q(x_true_i | y_i) by model.log_prob_pairs, both at the same step count and precision, then
    coverage_from_logq. (The samples' log q is integrated along their own reverse trajectory and the truths' along the
    forward grid: they agree to second order in 1 / num_steps.) Returns coverage_from_logq's dict plus logq_truth (n,)
    and logq_samples (n, num_samples), device tensors."""
    y = torch.as_tensor(y)
    if y.ndim != 2:
        raise ValueError("hpd_coverage: y must be (n, ydim), one observation per row of x_true")
    _, logq_s = model.sample_with_log_prob(y, num_samples, num_steps=num_steps, seed=seed, precision=precision)
    logq_t = model.log_prob_pairs(x_true, y, num_steps=num_steps, precision=precision)
    rep = coverage_from_logq(logq_t, logq_s, levels)
    rep.update(logq_truth=logq_t, logq_samples=logq_s)
    return rep
