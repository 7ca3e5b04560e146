"""The samplers' f32-accuracy gate, proved sharp on the CPU (no device): for every run of tests/accuracy_cases.py

  1. the float64 restatement (em_ref.py, heun_ref.py) and the fixture-pinned f32 oracle agree element-wise to 2e-6 and
     are not identical: a wrong sign, draw order or corrector in the restatement would miss by orders of magnitude;
  2. the emulated faithful three-product split passes the gate with at least 2x to spare;
  3. each emulated fault (a lost W_lo h_hi or W_hi h_lo, flushed lo subnormals, fp16 activations) exceeds it by at
     least 4x;
  4. the float64 chains at another beta_max miss it by at least 50x (as tests/test_sde_params_host.py asks of its cases).

These are conditions on the inputs, not tolerances to tune: a run that cannot show them is not in the gate
(accuracy_cases.py's docstring lists what that cost). `pytest -s` prints every run's separations.
"""
import numpy as np
import pytest

import accuracy_cases as A

AGREE = 2e-6
SPARE, EXCEED, MOVE = 2.0, 4.0, 50.0


@pytest.mark.parametrize("cid,S", A.RUNS)
def test_gate_is_sharp(dmip, cid, S):
    c = A.CASES[cid]
    r64, r32 = A.refs(dmip, cid, S)
    base, e_cpu = A.bound(dmip, cid, S)
    k = A.CASE_K.get(cid, A.K)
    assert k <= 16.0
    assert r64.dtype == np.float64 and r32.dtype == np.float32 and r64.shape == r32.shape == (c.n, c.xd)
    assert np.all(np.isfinite(r64)) and np.all(np.isfinite(r32))
    e_ok = A.err(A.emulated(dmip, cid, S), r64)
    print(f"{cid} S = {S}: max |ref| = {np.abs(r64).max():.4g}, err(f32) = {e_cpu:.3e}, faithful split "
          f"{e_ok / base:.2f} x")
    assert 0.0 < e_cpu <= AGREE, (cid, S, e_cpu)
    assert e_ok * SPARE <= k * base, (cid, S, e_ok, base)
    for fault in A.FAULTS:
        e = A.err(A.emulated(dmip, cid, S, fault), r64)
        print(f"    {fault}: {e / base:.1f} x")
        assert e >= EXCEED * k * base, (cid, S, fault, e, base)
    e = A.err(A.variant(dmip, cid, S), r64)
    print(f"    beta_max at the other SDE's: {e / base:.3g} x")
    assert e >= MOVE * k * base, (cid, S, e, base)


@pytest.mark.parametrize("cid", list(A.LEFT_OUT))
@pytest.mark.parametrize("S", [6, 50])
def test_left_out_case_still_pins_the_restatement(dmip, cid, S):
    """The predictor-corrector case is not in the gate (its faults do not separate), but em_ref's corrector is held to
    the oracle's on it, and moves the chains."""
    r64, r32 = A.refs(dmip, cid, S)
    e = A.err(r32, r64)
    print(f"{cid} S = {S}: err(f32) = {e:.3e}")
    assert 0.0 < e <= AGREE
    c = A.LEFT_OUT[cid]
    _, params, _, y, _ = A.model(dmip, cid)
    plain = A.EM.cdiffe_sample(params, y, c.n, S, A.SEED, **A._kw(c.sde))
    assert np.abs(plain - r64).max() > 1e-2


def test_the_emulation_without_a_fault_is_the_oracle_to_rounding(dmip):
    """split_mlp itself on one layer: its three products reproduce the float64 product to 2^-21 of sum |w h| (worst
    case: the dropped W_lo h_lo at 2^-22, the halves' own residual at 2^-22, the f32 rounding at 2^-24), and with a
    product lost (up to 2^-11 per term) they do not."""
    _, params, _, y, _ = A.model(dmip, "x3k-cde256-x3")
    g = np.random.default_rng(0)
    inp = np.concatenate([g.normal(size=(64, 3)), np.broadcast_to(y, (64, y.size)), np.full((64, 1), 0.37)], 1)
    inp = inp.astype(np.float32)
    W, b = params[0]
    exact = inp.astype(np.float64) @ W.astype(np.float64).T + b
    mag = np.abs(inp).astype(np.float64) @ np.abs(W).astype(np.float64).T + np.abs(b)
    one = [(W, b)]
    assert (np.abs(A.split_mlp(one, inp) - exact) / mag).max() < 2.0 ** -21
    for fault in ("no_w_lo", "no_h_lo"):
        assert (np.abs(A.split_mlp(one, inp, fault) - exact) / mag).max() > 2.0 ** -17
    assert np.array_equal(A.split_mlp(one, inp, "act_fp16"), A.split_mlp(one, inp))  # (a single layer has no activation)
