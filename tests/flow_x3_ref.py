"""Numpy f64 restatement of the algebra the fp32x3 flow kernels implement (csrc/dmip_x3_flow.h): the score network in
r-form with its forward tangents, folded here from the plain (W, b) of each layer. A plain module.

r-form: with c = 2 log2(e) and zs = c z, r = 1 / (1 + 2^zs) = (1 - tanh z) / 2, so h = tanh z = 1 - 2 r and every
layer after the first is affine in r:
    layer 1   A1 = c W1, i1 = c b1;  r1 = act(A1 inp + i1), r2 = act(c (1 - 2 r1))        (tanh(tanh z))
    hidden    A = -2 c W, i = c b - 1/2 sum_k A_k = c (b + sum_k W_k);  r = act(A r_prev + i)
    output    A = -2 Wo,  i = bo - 1/2 sum_k A_k;  a = A r + i
A tangent carries dr through the same A with no init:
    dr1 = -ln2 r1 (1 - r1) dzs with dzs = A1[:, n] for input n;  dr2 = -ln2 r2 (1 - r2) (-2 c dr1)
    hidden: dr = -ln2 r (1 - r) (A dr_prev);  output: da/dx_n = A dr, with no further factor.
(The kernel's fp16 split of every A and every r only rounds these numbers; it does not change the algebra.)
"""
import numpy as np

C = 2.0 * np.log2(np.e)
LN2 = np.log(2.0)


def fold(params):
    """[(A, init)] of every layer from the plain [(W, b)]: layer 1, the hidden layers, the output layer."""
    W = [np.asarray(p[0], np.float64) for p in params]
    b = [np.asarray(p[1], np.float64) for p in params]
    out = [(C * W[0], C * b[0])]
    for l in range(1, len(W) - 1):
        A = -2.0 * C * W[l]
        out.append((A, C * b[l] - 0.5 * A.sum(1)))
    A = -2.0 * W[-1]
    out.append((A, b[-1] - 0.5 * A.sum(1)))
    return out


def act_r(zs):
    return 1.0 / (1.0 + np.exp2(zs))


def dact_r(r):
    """dr / dzs at r = act_r(zs)."""
    return -LN2 * r * (1.0 - r)


def mlp_jet_rform(params, inp, d):
    """flow_ref.mlp_jet in r-form: a (n, out) and J[n, i, k] = da_i / d inp_k for the first d input columns."""
    L = fold(params)
    inp = np.asarray(inp, np.float64)
    A, i0 = L[0]
    zs = inp @ A.T + i0
    dzs = np.broadcast_to(A[None, :, :d], (inp.shape[0], A.shape[0], d))
    r1 = act_r(zs)
    dr1 = dact_r(r1)[:, :, None] * dzs
    r = act_r(C * (1.0 - 2.0 * r1))
    dr = dact_r(r)[:, :, None] * (-2.0 * C * dr1)
    for A, i0 in L[1:-1]:
        zs = r @ A.T + i0
        dzs = np.einsum("ij,njk->nik", A, dr)
        r = act_r(zs)
        dr = dact_r(r)[:, :, None] * dzs
    A, i0 = L[-1]
    return r @ A.T + i0, np.einsum("ij,njk->nik", A, dr)


def score_div_rform(params, x, y, tau, g, prior_params=None):
    """flow_ref.score_div through mlp_jet_rform: a(x, y, tau) (n, d) and sum_i da_i/dx_i (n,)."""
    x = np.asarray(x, np.float64)
    n, d = x.shape
    t = np.full((n, 1), tau, np.float64)
    yy = np.broadcast_to(np.asarray(y, np.float64), (n, np.asarray(y).shape[-1]))
    a, J = mlp_jet_rform(params, np.concatenate([x, yy, t], 1), d)
    dv = np.trace(J, axis1=1, axis2=2)
    if prior_params is not None:
        ap, Jp = mlp_jet_rform(prior_params, np.concatenate([x, t], 1), d)
        a, dv = g * (a + ap), g * (dv + np.trace(Jp, axis1=1, axis2=2))
    return a, dv
