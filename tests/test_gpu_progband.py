"""Banded profile-profile merges of `from_msa --unaligned --progressive --band` on the GPU (csrc/k_prog_band.inc), both backends:
tests/progband_common.py's checks against the plain-Python references (tests/progband_ref.py, tests/prog_ref.py)."""
import pytest

from tests import prog_common as pc
from tests import progband_common as pbc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=["runtime", "torch"])
def be(request):
    import torch  # noqa: F401  (before the library: HipBackend needs torch's HIP runtime to be the one the library binds)
    from make_prg_amd import backend as b
    return b.HipRuntimeBackend(0) if request.param == "runtime" else b.HipBackend(0)


def test_banded_kernel_equals_the_reference_banded_dp(be):
    pbc.check_kernel(be)


def test_widths_kernel_equals_the_linear_search(be):
    pbc.check_widths(be)


def test_two_pass_merges_equal_the_unbanded_results(be):
    pbc.check_two_pass_merges(be)


def test_tall_profiles_equal_the_unbanded_results(be):
    pc.check_tall_dp(be, band=True)


def test_msas_and_counters_equal_the_references(be):
    pbc.check_msas(be)


def test_compositions_with_adjust_direction_and_refine(be):
    pbc.check_compositions(be)


def test_certified_bands_give_the_full_dp(be):
    pbc.check_property(be)


def test_abi_statuses(be):
    pbc.check_abi_statuses(be)


def test_the_four_entries_of_the_sweep_agree_on_a_one_row_x(be):
    pbc.check_forms_agree(be)
