"""Static checks of the Metropolis-adjusted Langevin kernel in the built gfx950 code object (CPU only): both
instantiations of mala_kernel (product RNG, injected draws) are there, call no outlined device function and need no
dynamic stack -- the conditions tests/test_isa.py holds every kernel to, on its `isa` fixture."""
from test_isa import isa  # noqa: F401 -- the fixture


def test_mala_kernel_found_inlined_and_on_a_static_stack(isa):
    kernels = {k: v for k, v in isa.items() if "mala_kernel" in k}
    assert len(kernels) == 2, sorted(kernels)
    bad = {k: v for k, v in kernels.items() if v.get("calls", 0) or v.get("uses_dynamic_stack")}
    assert not bad, bad
