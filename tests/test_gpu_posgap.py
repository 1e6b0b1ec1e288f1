"""Position-specific gap opens of `from_msa --unaligned --progressive --position-gaps` on the GPU (csrc/pg_pairs.inc,
csrc/pg_pairs_band.inc, csrc/pg_band_widths.inc), both backends: tests/posgap_common.py's checks against the plain-Python
statement (tests/posgap_ref.py)."""
import pytest

from tests import posgap_common as pgc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=["runtime", "torch"])
def be(request):
    import torch  # noqa: F401  (before the library: HipBackend needs torch's HIP runtime to be the one the library binds)
    from make_prg_amd import backend as b
    return b.HipRuntimeBackend(0) if request.param == "runtime" else b.HipBackend(0)


def test_dp_kernel_equals_the_reference(be):
    pgc.check_dp(be)


def test_gap_free_sides_equal_the_fixed_open_entry(be):
    pgc.check_gap_free(be)


def test_tall_profiles_and_opens_that_do_not_divide(be):
    pgc.check_tall_and_divisors(be)


def test_seventh_plane_and_unchanged_kinds(be):
    pgc.check_planes(be)


def test_banded_kernel_equals_the_reference_banded_dp(be):
    pgc.check_kernel(be)


def test_widths_kernel_equals_the_linear_search(be):
    pgc.check_widths(be)


def test_two_pass_merges_equal_the_unbanded_results(be):
    pgc.check_two_pass_merges(be)


def test_certified_bands_give_the_full_dp(be):
    pgc.check_property(be)


def test_msas_equal_the_reference_with_band_and_device_tree(be):
    pgc.check_same_bytes(be)


def test_compositions_with_collapse_seq_weights_retree_and_refine_tree(be):
    pgc.check_compositions(be)


def test_refine_afterwards_is_refine_ref_on_the_new_rows(be):
    pgc.check_refine_afterwards(be)


def test_flag_off_gives_prog_ref(be):
    pgc.check_flag_off(be)


def test_the_finding_on_the_device(be):
    pgc.check_finding(be)


def test_abi_statuses(be):
    pgc.check_abi_statuses(be)


def test_from_msa_position_gaps_writes_the_reference_files(be, tmp_path, caplog):
    pgc.check_cli(be, tmp_path, caplog)
