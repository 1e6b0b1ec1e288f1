"""Free end distances, `from_msa --unaligned --progressive --pair-distances --free-end-distances`, on the MI355X through both backends:
mprg_align_pair_scores_endgap and mprg_align_pair_scores_endgap_banded against the plain DPs, against mprg_align_pairs_endgap on the
same tables and against the charged kernels (the shapes around the 64-row strip and the 128-column ring, leaves of 1 and 3 rows, guard
words), their refusals, the host's two passes, whole MSAs against tests/freedist_ref.py (the four fragment loci of the finding
among them), the compositions with the other flags, what moves between host and device, and the command line in process
(tests/freedist_common.py holds the checks)."""
import pytest

from tests import freedist_common as fc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=["runtime", "torch"])
def backend(request):
    import torch  # noqa: F401  (before the library: HipBackend needs torch's HIP runtime to be the one the library binds)
    from make_prg_amd import backend as b
    return b.HipRuntimeBackend(0) if request.param == "runtime" else b.HipBackend(0)


def test_score_kernel_equals_the_dp(backend):
    fc.check_kernel(backend)


def test_banded_score_kernel_equals_the_banded_dp(backend):
    fc.check_banded_kernel(backend)


def test_refusals(backend):
    fc.check_refusals(backend)


def test_two_passes_return_the_full_scores(backend):
    fc.check_two_pass(backend)


def test_msas_equal_the_statement(backend):
    fc.check_msas(backend)


def test_band_device_tree_and_small_budgets_give_the_same_bytes(backend):
    fc.check_same_bytes(backend)


def test_default_band_device_tree_and_small_budgets_on_the_fragment_loci(backend):
    fc.check_same_bytes_msa_loci(backend)


def test_compositions(backend):
    fc.check_compositions(backend)


def test_compositions_on_the_fragment_loci(backend):
    fc.check_compositions_msa_loci(backend)


def test_flag_off_and_what_moves(backend):
    fc.check_trace(backend)


def test_parameters(backend):
    fc.check_parameters(backend)


def test_command_line(backend, tmp_path, caplog):
    fc.check_cli(backend, tmp_path, caplog)
