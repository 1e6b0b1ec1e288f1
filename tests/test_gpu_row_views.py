"""GPU twin of tests/test_row_views_emulated.py: the narrow views of mprg_ungap_dedupe (k_rows_narrow) on the MI355X against the
oracle — the barrier between the row phase and the dedupe, the workgroup's stores read back by its other lanes and many workgroups
at once are only seen here.  (The test-only weak-hash build exists for the emulator alone.)  Run with `-m gpu`."""
import pytest

from tests import parity_common as pc
from tests import row_view_cases as rv

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rt():
    import torch  # noqa: F401  (before the library: a later HipBackend needs torch's HIP runtime to be the one the library binds)
    from make_prg_amd.backend import HipRuntimeBackend
    return HipRuntimeBackend(0)


@pytest.fixture(autouse=True)
def forest_host(monkeypatch):
    monkeypatch.setattr(pc, "ENGINE", "forest")


@pytest.mark.parametrize("col0_mod", [0, 1, 2, 3])
def test_widths(rt, col0_mod):
    pc.check_vs_oracle(rt, *rv.widths(col0_mod))


def test_heights(rt):
    pc.check_vs_oracle(rt, *rv.heights())


@pytest.mark.parametrize("L", [7, 3])
def test_row_content(rt, L):
    pc.check_vs_oracle(rt, *rv.row_content(L))


def test_identical_rows(rt):
    pc.check_vs_oracle(rt, *rv.identical_rows())


@pytest.mark.parametrize("L", [3, 7])
def test_kmer_boundary(rt, L):
    pc.check_vs_oracle(rt, *rv.kmer_boundary(L))


def test_mixed_batch(rt):
    pc.check_vs_oracle(rt, *rv.mixed_batch())
