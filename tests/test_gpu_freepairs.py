"""Free end pairs of `from_msa --unaligned --free-end-pairs` on the GPU (csrc/al_pairs.inc, csrc/al_pairs_band.inc,
k_align_bounds_endgap in csrc/k_align.inc), both backends: tests/freepairs_common.py's checks against the plain-Python statement
(tests/freepairs_ref.py)."""
import pytest

from tests import freepairs_common as fpc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=["runtime", "torch"])
def be(request):
    import torch  # noqa: F401  (before the library: HipBackend needs torch's HIP runtime to be the one the library binds)
    from make_prg_amd import backend as b
    return b.HipRuntimeBackend(0) if request.param == "runtime" else b.HipBackend(0)


def test_dp_kernel_equals_the_reference_and_the_profile_pair_entry(be):
    fpc.check_dp(be)


def test_banded_kernel_equals_the_reference_banded_dp(be):
    fpc.check_banded(be)


def test_bounds_kernel_equals_python(be):
    fpc.check_bounds(be)


def test_two_passes_equal_the_unbanded_results(be):
    fpc.check_two_pass(be)


def test_abi_statuses(be):
    fpc.check_abi_statuses(be)


def test_star_msas_equal_the_reference_with_band_collapse_and_adjust_direction(be):
    fpc.check_star(be)


def test_refine_rounds_and_objective_are_the_references(be):
    fpc.check_refine(be)


def test_progressive_with_free_end_gaps_and_refine_and_the_star_fallback(be):
    fpc.check_progressive(be)


def test_a_unique_substring_of_the_centre_lies_in_place(be):
    fpc.check_unique_substring(be)


def test_flag_off_gives_star_ref_and_refine_ref(be):
    fpc.check_flag_off(be)


def test_the_finding_on_the_device(be):
    fpc.check_finding(be)


def test_from_msa_free_end_pairs_writes_the_reference_files(be, tmp_path, caplog):
    fpc.check_cli(be, tmp_path, caplog)
