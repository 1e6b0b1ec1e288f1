"""Free end gaps of `from_msa --unaligned --progressive --free-end-gaps` on the GPU (csrc/pg_pairs.inc, csrc/pg_pairs_band.inc,
csrc/pg_band_widths.inc), both backends, both forms of the open: tests/endgap_common.py's checks against the plain-Python statement
(tests/endgap_ref.py)."""
import pytest

from tests import endgap_common as egc

pytestmark = pytest.mark.gpu

OPENS = pytest.mark.parametrize("posgap", [False, True], ids=["fixed", "posgap"])


@pytest.fixture(scope="module", params=["runtime", "torch"])
def be(request):
    import torch  # noqa: F401  (before the library: HipBackend needs torch's HIP runtime to be the one the library binds)
    from make_prg_amd import backend as b
    return b.HipRuntimeBackend(0) if request.param == "runtime" else b.HipBackend(0)


@OPENS
def test_dp_kernel_equals_the_reference(be, posgap):
    egc.check_dp(be, posgap)


@OPENS
def test_tall_profiles(be, posgap):
    egc.check_tall(be, posgap)


@OPENS
def test_banded_kernel_equals_the_reference_banded_dp(be, posgap):
    egc.check_kernel(be, posgap)


def test_widths_kernel_equals_the_linear_search(be):
    egc.check_widths(be)


@OPENS
def test_two_pass_merges_equal_the_unbanded_results(be, posgap):
    egc.check_two_pass_merges(be, posgap)


@OPENS
def test_msas_equal_the_reference_with_band_and_device_tree(be, posgap):
    egc.check_same_bytes(be, posgap)


@OPENS
def test_compositions_with_collapse_seq_weights_retree_refine_tree_and_large_loci(be, posgap):
    egc.check_compositions(be, posgap)


@OPENS
def test_refine_afterwards_is_refine_ref_on_the_new_rows(be, posgap):
    egc.check_refine_afterwards(be, posgap)


def test_flag_off_gives_prog_ref(be):
    egc.check_flag_off(be)


def test_the_finding_on_the_device(be):
    egc.check_finding(be)


def test_abi_statuses(be):
    egc.check_abi_statuses(be)


def test_from_msa_free_end_gaps_writes_the_reference_files(be, tmp_path, caplog):
    egc.check_cli(be, tmp_path, caplog)
