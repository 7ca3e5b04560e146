"""reference `models.SNF`: `energy_grad` (models/SNF.py:234-237), which the scatterometry driver imports
for the posterior score; `anneal_to_energy` (models/SNF.py:250-275), the Metropolis-Hastings sampler that
generate_scatterometry_ground_truth.py imports, with random-walk or Langevin proposals (fused on the device for a
ScatterometryEnergy); and the helpers of its Langevin branch, `langevin_step` (models/SNF.py:286-300) and
`get_interpolated_energy_fun` (models/SNF.py:220-231). The SNF baseline's networks are out of scope."""
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from _base import export  # noqa: E402
export(globals(), "problems", ["energy_grad", "anneal_to_energy", "langevin_step", "get_interpolated_energy_fun"])
