"""The k-major fp32x3 CDE sampler (csrc/dmip_x3k.h) reproduces its recorded output bit for bit.

tests/golden/x3k_bits.npz holds `CDE.sample_device(..., precision="fp32x3")` at hidden_layers [256]*3 from the build
of the commit before the step loop's accumulator traffic was cut (tests/golden/make_x3k_bits.py records it and
defines the cases, so the two cannot drift apart). Changes of that kind move or copy values and re-associate no sum:
`np.array_equal`, no tolerance. Needs an MI355X: `pytest -m gpu`.

Cases (the smallest at which this code can go wrong; a few milliseconds each): (xdim, ydim) = (3, 23) and (2, 2);
49 and 97 chains (a ragged last job, a partly empty tile); 17 steps (no multiple of the ring period); two observations
in one launch; chain_offset shards (two halves are the whole); snapshots every 4 steps; DMIP_X3K_NT = 1 and 2 (the
8-wave form has other piece and barrier counts); one hand-over launch of 49,200 chains x 5 steps (more jobs than
resident waves: segment kinds 1, 2 and 3), compared on every 97th chain and the SHA-256 of the whole array.
"""
import importlib.util
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location("make_x3k_bits", os.path.join(GOLDEN, "make_x3k_bits.py"))
bits = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(bits)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


@pytest.fixture(scope="module")
def recorded():
    return np.load(os.path.join(GOLDEN, "x3k_bits.npz"))


@pytest.fixture(scope="module")
def models():
    return {}  # shape -> (model, observations), built once (make_x3k_bits.model_and_y)


def test_fixture_holds_every_case(recorded):
    have = {k.split("/")[0] for k in recorded.files if k != "meta"}
    assert have == {c["id"] for c in bits.CASES}


@pytest.mark.parametrize("case", bits.CASES, ids=[c["id"] for c in bits.CASES])
def test_x3k_bits(dmip, recorded, models, case):
    got = bits.run_case(dmip, models, case)
    dmip._lib.device_status("cuda:0")
    for name, arr in got.items():
        ref = recorded[f"{case['id']}/{name}"]
        assert arr.dtype == ref.dtype and arr.shape == ref.shape, (name, arr.dtype, arr.shape, ref.shape)
        assert np.array_equal(arr, ref), f"{case['id']}/{name}: {int((arr != ref).sum())} of {arr.size} elements differ"
