"""Free end distances, `from_msa --unaligned --progressive --pair-distances --free-end-distances` (make_prg_amd/from_msa/star_align.py
"Free end distances", csrc/al_scores.inc, csrc/al_scores_band.inc), on the CPU emulation build: the plain-Python statement against
itself and against the finding's table, mprg_align_pair_scores_endgap and mprg_align_pair_scores_endgap_banded called directly
(shapes, bands, guard words, refusals), the host's two passes, whole MSAs against the statement, the compositions with the other
flags, what moves between host and device, and the command line (tests/freedist_common.py holds the checks)."""
import pytest

from tests import freedist_common as fc
from tests.emu.backend import EmuBackend


@pytest.fixture(scope="module")
def emu():
    return EmuBackend()


# ---- the statement against itself
def test_the_statement_keeps_its_four_facts():
    fc.check_statement()


def test_an_exact_substring_is_at_distance_zero():
    fc.check_substrings()


def test_the_statement_reproduces_the_table():
    fc.check_table()


def test_the_banded_cases_meet_their_conditions():
    fc.check_banded_conditions()


def test_the_two_pass_locus_takes_every_route():
    fc.check_two_pass_conditions()


def test_the_references_give_the_recorded_finding():
    fc.check_finding_reference()


# ---- the kernels
def test_score_kernel_equals_the_dp(emu):
    fc.check_kernel(emu)


def test_banded_score_kernel_equals_the_banded_dp(emu):
    fc.check_banded_kernel(emu)


def test_refusals(emu):
    fc.check_refusals(emu)


def test_two_passes_return_the_full_scores(emu):
    fc.check_two_pass(emu)


# ---- whole MSAs
def test_msas_equal_the_statement(emu):
    fc.check_msas(emu)


def test_band_device_tree_and_small_budgets_give_the_same_bytes(emu):
    fc.check_same_bytes(emu)


def test_default_band_device_tree_and_small_budgets_on_the_fragment_loci(emu):
    fc.check_same_bytes_msa_loci(emu)


def test_compositions(emu):
    fc.check_compositions(emu)


def test_compositions_on_the_fragment_loci(emu):
    fc.check_compositions_msa_loci(emu)


def test_flag_off_and_what_moves(emu):
    fc.check_trace(emu)


def test_parameters(emu):
    fc.check_parameters(emu)


# ---- the command line
def test_parser(capsys):
    fc.check_parser(capsys)


def test_command_line(emu, tmp_path, caplog):
    fc.check_cli(emu, tmp_path, caplog)
