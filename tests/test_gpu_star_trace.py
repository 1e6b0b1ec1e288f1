"""tests/test_star_trace_emulated.py on the MI355X: the DP is integer and the host code the same, so the HIP backend is asked
exactly what the emulation is asked and gives the same MSAs: the same digests (tests/golden/star_trace.json)."""
import pytest

from tests import star_trace as tr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def backend():
    import torch  # noqa: F401  (before the library: HipBackend needs torch's HIP runtime to be the one the library binds)
    from make_prg_amd import backend as b
    return b.HipRuntimeBackend(0)


@pytest.mark.parametrize("name", list(tr.scenarios()))
def test_trace_equals_the_golden(backend, name):
    assert tr.run(backend, name)[1] == tr.golden()[name]
