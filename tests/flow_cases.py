"""The cases of the density kernels' accuracy gate: what tests/test_gpu_flow_x3.py and tests/test_gpu_pairs.py run on the
device and tests/test_flow_accuracy_host.py proves sharp on the CPU. A plain module beside accuracy_cases.py: inputs,
cached read-only restatements, the gate and a numpy emulation of the split engine's tangent path; nothing here touches
the device.

The claim under test: log_prob and sample_with_log_prob (and their _pairs forms) integrate the score
network's exact divergence, which on the fp32x3 engine comes from forward tangents through the split-fp16 products.
The tangent columns dr are split into (hi, lo) fp16 like any activation and pass through A = [W_hi, W_hi, W_lo]; at
layer 1 they come from a unit-vector B operand whose k-slot 3n + 2 brings in W_lo. The primal columns are the
samplers' chains (accuracy_cases.py holds those); the faults emulated here touch tangent operands only.

Gate, per output (logp and latent of log_prob, logq and x of sample_with_log_prob), on the absolute error:
    e_gpu <= K max(e_cpu, 1e-7),   K = 8
with e_gpu = max |gpu - f64| and e_cpu = max |f32 restatement - f64| over the same rows, the f32 side being the
restatement's own f32 run (flow_ref.log_prob, flow_sample_ref.sample_with_logq), never a kernel. It replaces
    e_gpu <= 4 e_cpu + 1e-6 max(1, max |f64|)                                        (`old_tol`)
whose second term on logp is 35 to 42 e_cpu at W 512: an emulated kernel that drops W_lo dr_hi, drops W_hi dr_lo or
flushes the lo subnormals in every layer passes it there (tests/test_flow_accuracy_host.py pins that). K: the
faithful emulation lands at 0.6-1.6 of max(e_cpu, 1e-7) on logp and logq (2.4 at most on a latent), the weakest
all-layer fault of any case at 21.7 (W 512, the default SDE; THIN below); the device was measured at 0.3 to 3.68 but
for the three gates of CASE_K. 8 leaves 2x over the worst of those and 2x under the weakest fault; the
host test asserts both margins on every case. A gate whose device ratio above K / 2 is a documented property of the
arithmetic carries its own K (twice the measured ratio, never above 16) in CASE_K by the gate's printed name, with
the cause in DESIGN.md 3g.

No assertion became looser: where e_cpu is large (the trained fixtures: logp e_cpu 3e-6 to 7e-6 over 6 to 20 steps),
8 e_cpu exceeds the old 4 e_cpu + 1e-6, so the tolerance is the smaller of the two (`tolerance`); the old bound
binds on those arrays and K max(e_cpu, 1e-7) on all others (the host test prints which, and asserts tol <= old).

Cases: the seeded shapes of tests/test_gpu_flow_x3.py (SHAPES: oracle.reference_weights networks, rows
heun_ref.x0_of_seed(seed), y = default_rng(seed).normal(size=(3, ydim))[0], S = 4, the default VP-SDE) and the trained
fixture cases a / b / d of tests/golden/flow_logp.npz (ckpt_lin 37 rows S = 20; ckpt_scat, its first 37 rows, S = 10;
the Posterior pair, 21 rows x 2 ys, S = 6, where the divergence is g (dv + dv_prior) over two networks), and the
paired form of each seeded shape and of d with a different y in every row. sample_with_log_prob always gets x0
injected: the rows themselves for the seeded shapes, heun_ref.x0_of_seed(1234, n, xdim, stream = y index) for the
fixtures.

Left out of the fault margins (INSIDE): a single-site fault that stays inside the gate on a case, with the measured
value, as accuracy_cases.LEFT_OUT does for the samplers.
"""
import collections
import contextlib
import functools

import numpy as np

import flow_ref as FR
import flow_sample_ref as FS
import flow_x3_ref as X3
import heun_ref as HR
import oracle as O
from conftest import GOLDEN

F16, F32, F64 = np.float16, np.float32, np.float64
K = 8.0
FLOOR = 1e-7
# {the gate's printed name: its own K}, twice the device's measured ratio (DESIGN.md 3g has the causes)
CASE_K = {
    # one row: e_cpu is that row's own 4.5e-8, under the floor; the same e_gpu 5.17e-7 is 1.80 over three rows
    "w64 n=1 fp32 logp": 10.34,
    "w64 n=1 fp32x3 logp": 10.34,
    # five rows at the SDE (1.1, 25, 1.25): the split engine's primal error on a latent of |x| <= 0.81, 5.90 (the
    # exact-f32 kernel: 1.45); the replaced gate's tolerance, 7.36 e_cpu, is the one in force there
    "SDE B post64 fp32x3 latent": 11.8,
}
SCHEMES = ("logp", "sample")   # log_prob: arrays (logp, latent); sample_with_log_prob, x0 injected: arrays (logq, x)
ARRAYS = {"logp": ("logp", "latent"), "sample": ("logq", "x")}
ALL_LAYER = ("t_no_w_lo", "t_no_h_lo", "t_flush_lo")
SINGLE_SITE = ("t_l1_no_lo", "t_out_no_w_lo")
FAULTS = ALL_LAYER + SINGLE_SITE

SHAPES = {  # name: (W, n_hidden, xdim, ydim, rows of the shared reference, weight seed); S = 4
    "w64": (64, 3, 2, 2, 37, 301),
    "w128": (128, 3, 2, 2, 19, 302),
    "w64x1": (64, 1, 3, 5, 21, 305),
    "w512": (512, 3, 3, 23, 21, 304),
}
S_SEEDED = 4
FIXTURES = ("a", "b", "d")
MAX_ROWS = 37
X0_SEED = 1234
PAIRED = {f"{name}-pairs": name for name in list(SHAPES) + ["d"]}
CASES = list(SHAPES) + list(FIXTURES) + list(PAIRED)
SEEDED_CASES = [c for c in CASES if PAIRED.get(c, c) in SHAPES]
FIXTURE_CASES = [c for c in CASES if c not in SEEDED_CASES]

# W 512 paired: its all-layer faults are held to K, not to 2 K. At W 512, S = 4 and the default SDE (|x| grows to 190,
# the layers saturate) the weakest all-layer fault of sample_with_log_prob lands at 10.7 to 19.7 of max(e_cpu, 1e-7)
# over five draws of the rows' ys (17.1 at the draw used; the unpaired case of SHAPES: 21.7), so 2 K = 16 is met
# or missed by the draw; every draw is beyond K. The single-site faults at W 512 (6.5 to 30, paired and unpaired) are
# printed and not asserted: they are asserted at W 64 and W 128 and on the fixtures.
THIN = ("w512-pairs",)
W512 = ("w512", "w512-pairs")

# (case, scheme, fault): a single-site fault that stays inside the gate there, with the measured e / max(e_cpu, 1e-7)
# in the comment; at most two. The host test asserts they are still inside (so the list cannot go stale).
INSIDE = {}

# one run of a restatement: rows x (n, d), y (ydim,) or one y per row (n, ydim), the x0 of sample_with_log_prob
Run = collections.namedtuple("Run", "x y x0")
Data = collections.namedtuple("Data", "params prior runs S")


def _ro(a):
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


def _golden(name):
    return np.load(f"{GOLDEN}/{name}")


@functools.lru_cache(maxsize=None)
def _networks(name):
    """(likelihood or CDE params, prior params or None) of a seeded shape or a fixture case."""
    if name in SHAPES:
        W, NL, xd, yd, _, seed = SHAPES[name]
        return tuple(O.reference_weights([xd + yd + 1] + [W] * NL + [xd], seed)), None
    if name == "a":
        return tuple(O.mlp_params_from_state(_golden("ckpt_lin.npz"))), None
    if name == "b":
        return tuple(O.mlp_params_from_state(_golden("ckpt_scat.npz"))), None
    return (tuple(O.mlp_params_from_state(_golden("posterior_loss.npz"), "lik_")),
            tuple(O.mlp_params_from_state(_golden("ckpt_prior_scat.npz"))))


@functools.lru_cache(maxsize=None)
def data(cid):
    """Data(params, prior, runs, S) of a case, read-only. A case's outputs are its runs' outputs, concatenated."""
    name = PAIRED.get(cid, cid)
    params, prior = _networks(name)
    if name in SHAPES:
        W, NL, xd, yd, n, seed = SHAPES[name]
        x = HR.x0_of_seed(seed, n, xd)
        if cid in PAIRED:
            y = np.random.default_rng(seed + 1000).normal(size=(n, yd)).astype(F32)
        else:
            y = np.random.default_rng(seed).normal(size=(3, yd)).astype(F32)[0]
        return Data(params, prior, (Run(_ro(x), _ro(y), _ro(x)),), S_SEEDED)
    z = _golden("flow_logp.npz")
    S = int(z[f"{name}_S"])
    if cid in PAIRED:   # d's first rows, every row under an observation of its own around d's first
        x = z["d_x"][0]
        y = (z["d_y"][0] + 0.25 * np.random.default_rng(256).normal(size=(len(x), z["d_y"].shape[1]))).astype(F32)
        return Data(params, prior, (Run(_ro(x), _ro(y), _ro(HR.x0_of_seed(X0_SEED, len(x), x.shape[1]))),), S)
    xs, ys = (z[f"{name}_x"], z[f"{name}_y"])
    if xs.ndim == 2:
        xs, ys = xs[None, :MAX_ROWS], ys[None]
    runs = tuple(Run(_ro(x), _ro(y), _ro(HR.x0_of_seed(X0_SEED, len(x), x.shape[1], stream=i)))
                 for i, (x, y) in enumerate(zip(xs, ys)))
    return Data(params, prior, runs, S)


@contextlib.contextmanager
def _blas_einsum():
    """flow_ref's contractions through numpy's BLAS path: the same sums in another order, far faster (as
    tests/test_gpu_flow_x3.py test_consistent_with_log_prob_to_second_order). For the f64 run only: e_cpu is the f32
    run's error with flow_ref's own sums, one after the other as the kernels' accumulators take them; BLAS's blocked
    f32 sums round less (case d, logp: e_cpu 2.9e-6 against 5.1e-6) and would measure the kernels against a
    different arithmetic."""
    saved = np.einsum
    np.einsum = functools.partial(saved, optimize=True)
    try:
        yield
    finally:
        np.einsum = saved


def _one_blas_thread():
    """These products are small (at most 37 rows): a threaded BLAS spends its time handing them out. Speed only."""
    try:
        import threadpoolctl
    except ImportError:
        return contextlib.nullcontext()
    return threadpoolctl.threadpool_limits(limits=1, user_api="blas")


def _run(cid, scheme, dtype, blas=True):
    with _blas_einsum() if blas else contextlib.nullcontext(), _one_blas_thread():
        return _run_plain(cid, scheme, dtype)


def _run_plain(cid, scheme, dtype):
    d = data(cid)
    out = []
    for r in d.runs:
        if scheme == "logp":
            logp, lat = FR.log_prob(list(d.params), r.x, r.y, d.S, d.prior and list(d.prior), dtype=dtype)
            out.append((logp, lat))
        else:
            x, logq = FS.sample_with_logq(list(d.params), r.x0, r.y, d.S, d.prior and list(d.prior), dtype=dtype)
            out.append((logq, x))
    return {name: _ro(np.concatenate([o[i] for o in out])) for i, name in enumerate(ARRAYS[scheme])}


@functools.lru_cache(maxsize=None)
def refs(cid, scheme):
    """({array: f64 restatement}, {array: its f32 run}) of the case under the scheme, read-only."""
    return _run(cid, scheme, F64), _run(cid, scheme, F32, blas=False)


# ------------------------------------------------------------------------------------------ the split engine, emulated
def _halves(v, flush=False):
    v = np.asarray(v, F64)
    hi = v.astype(F16).astype(F64)
    lo = (v - hi).astype(F16).astype(F64)   # (numpy's fp16 keeps its subnormals)
    if flush:
        lo = np.where(np.abs(lo) < 2.0 ** -14, 0.0, lo)
    return hi, lo


_folded = {}   # {id of the network's first weight: [(A_hi, A_lo, A_lo flushed, init)]}: the weights, split once per run


def _fold(params):
    key = id(params[0][0])
    if key not in _folded:
        layers = []
        for A, init in X3.fold(params):
            hi, lo = _halves(A)
            layers.append((hi, lo, _halves(A, flush=True)[1], init))
        _folded[key] = (params[0][0], layers)   # (the array is kept, so its id stays its own)
    return _folded[key][1]


def _f32(v):
    return np.asarray(v, F64).astype(F32).astype(F64)


def _three(a_hi, a_lo, h_hi, h_lo, w_lo=True, h_lo_term=True):
    """A_hi h_hi + A_hi h_lo + A_lo h_hi in f64; h is (n, k) (a primal) or (n, k, d) (its tangents)."""
    if h_hi.ndim == 2:
        mm = lambda A, h: h @ A.T  # noqa: E731
    else:   # one product over all rows' tangent columns
        n, k, d = h_hi.shape
        mm = lambda A, h: (A @ h.transpose(1, 0, 2).reshape(k, n * d)).reshape(-1, n, d).transpose(1, 0, 2)  # noqa: E731
    z = mm(a_hi, h_hi)
    if h_lo_term:
        z = z + mm(a_hi, h_lo)
    if w_lo:
        z = z + mm(a_lo, h_hi)
    return z


def split_jet(params, inp, d, fault=None):
    """flow_x3_ref.mlp_jet_rform as the split engine evaluates it, as an error class and not as the kernel: folded
    weights and r, dr in fp16 hi / lo halves with the subnormals kept, every layer A_hi h_hi + A_hi h_lo + A_lo h_hi
    summed in f64 and rounded once to f32, the activation and its tangent factor rounded to f32, the layer-1 tangent
    (A_hi + A_lo)[:, n]. Returns a (n, out) and J[n, i, k] = da_i / d inp_k, both f32 values.

    fault (tangent operands only; the primal columns are always faithful):
      t_no_w_lo      A_lo dr_hi dropped in every layer (layer 1: the unit vector's A_lo slot)
      t_no_h_lo      A_hi dr_lo dropped in every layer (dr rounded to fp16; layer 1's unit vector has no lo half)
      t_flush_lo     the lo halves of dr and of A below fp16's smallest normal 2^-14 flushed to zero
      t_l1_no_lo     the layer-1 tangent without its A_lo slot, nothing else
      t_out_no_w_lo  the output layer's A_lo dr_hi dropped, nothing else"""
    assert fault is None or fault in FAULTS, fault
    L = _fold(params)
    flush = fault == "t_flush_lo"
    keep_h_lo = fault != "t_no_h_lo"
    inp = np.asarray(inp, F32)
    # layer 1
    a_hi, a_lo, a_lo_fl, init = L[0]
    zs = _f32(_three(a_hi, a_lo, *_halves(inp)) + init)
    if fault in ("t_no_w_lo", "t_l1_no_lo"):
        col = a_hi[:, :d]
    else:
        col = a_hi[:, :d] + (a_lo_fl if flush else a_lo)[:, :d]
    dzs = np.broadcast_to(_f32(col)[None], (inp.shape[0],) + col.shape)
    r1 = _f32(X3.act_r(zs))
    dr1 = _f32(X3.dact_r(r1)[:, :, None] * dzs)
    r = _f32(X3.act_r(_f32(X3.C * (1.0 - 2.0 * r1))))
    dr = _f32(X3.dact_r(r)[:, :, None] * _f32(-2.0 * X3.C * dr1))
    # hidden layers, then the output layer (no activation, no tangent factor)
    for li, (a_hi, a_lo, a_lo_fl, init) in enumerate(L[1:], 1):
        last = li == len(L) - 1
        keep_w_lo = not (fault == "t_no_w_lo" or (last and fault == "t_out_no_w_lo"))
        zs = _f32(_three(a_hi, a_lo, *_halves(r)) + init)
        dzs = _f32(_three(a_hi, a_lo_fl if flush else a_lo, *_halves(dr, flush), w_lo=keep_w_lo, h_lo_term=keep_h_lo))
        if last:
            return zs.astype(F32), dzs.astype(F32)
        r = _f32(X3.act_r(zs))
        dr = _f32(X3.dact_r(r)[:, :, None] * dzs)


def _split_score_div(fault):
    """flow_ref.score_div in f32 with its networks evaluated by split_jet(fault)."""
    def score_div(params, x, y, tau, g, prior_params=None, dtype=F32):
        assert dtype == F32
        n, d = x.shape
        t = np.full((n, 1), tau, F32)
        yy = np.broadcast_to(np.asarray(y, F32), (n, np.asarray(y).shape[-1]))
        a, J = split_jet(params, np.concatenate([x, yy, t], 1), d, fault)
        dv = np.trace(J, axis1=1, axis2=2)
        if prior_params is not None:
            ap, Jp = split_jet(prior_params, np.concatenate([x, t], 1), d, fault)
            a, dv = g * (a + ap), g * (dv + np.trace(Jp, axis1=1, axis2=2))
        return a.astype(F32), dv.astype(F32)
    return score_div


@contextlib.contextmanager
def _emulated_networks(fault):
    """The restatements with every network evaluation replaced by split_jet; the steps and the f64 sums stay theirs."""
    saved = FR.score_div
    FR.score_div = _split_score_div(fault)
    try:
        yield
    finally:
        FR.score_div = saved


@functools.lru_cache(maxsize=None)
def emulated(cid, fault=None):
    """{scheme: {array: the f32 restatement's run with its networks evaluated by split_jet(fault)}}, both schemes."""
    with _emulated_networks(fault):
        return {scheme: _run(cid, scheme, F32) for scheme in SCHEMES}


# ------------------------------------------------------------------------------------------ the gate
def err(a, r64):
    return float(np.abs(np.asarray(a, F64) - np.asarray(r64, F64)).max())


def old_tol(ref64, ref32, scaled=True):
    """The gate this one replaces: 4 e_cpu + 1e-6 max(1, max |f64|) (`scaled`; else + 1e-6)."""
    ref64 = np.asarray(ref64, F64)
    return 4.0 * err(ref32, ref64) + 1e-6 * (max(1.0, float(np.abs(ref64).max())) if scaled else 1.0)


def tolerance(ref64, ref32, k=K, scaled=True):
    """(tol, base, e_cpu): base = max(e_cpu, 1e-7), tol = k base, and never above the old gate's tolerance at the
    caller's `scaled` (the module docstring says where that binds)."""
    e_cpu = err(ref32, ref64)
    base = max(e_cpu, FLOOR)
    return min(k * base, old_tol(ref64, ref32, scaled)), base, e_cpu


def gate(name, got, ref64, ref32, scaled=True, tag=""):
    """Assert e_gpu <= tolerance; prints the gate's ratio e_gpu / max(e_cpu, 1e-7) (`pytest -s`)."""
    k = CASE_K.get(name, K)
    assert k <= 16.0
    got, ref64 = np.asarray(got, F64), np.asarray(ref64, F64)
    tol, base, e_cpu = tolerance(ref64, ref32, k, scaled)
    e_gpu = err(got, ref64)
    print(f"{tag}{name}: e_gpu = {e_gpu:.3e}, e_cpu = {e_cpu:.3e}, ratio = {e_gpu / base:.2f} (K = {k:g}), "
          f"max |ref| = {np.abs(ref64).max():.4g}, tol = {tol:.3e}{'' if tol == k * base else ' (the old gate binds)'}")
    assert np.all(np.isfinite(got))
    assert e_gpu <= tol, (name, e_gpu, e_cpu, tol)
