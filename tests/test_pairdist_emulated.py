"""Pair distances, `from_msa --unaligned --progressive --pair-distances` (make_prg_amd/from_msa/star_align.py "Pair distances",
csrc/k_align_scores.inc), on the CPU emulation build: the plain-Python statement against itself, mprg_align_pair_scores and
mprg_align_pair_scores_banded called directly (shapes, bands, guard words, refusals), the host's two passes, the tables through the
tree entry points, the saturated locus, whole MSAs against the statement, the compositions with the other flags, what moves between
host and device, and the parser (tests/pairdist_common.py holds the checks)."""
import pytest

from tests import pairdist_common as pc
from tests.emu.backend import EmuBackend


@pytest.fixture(scope="module")
def emu():
    return EmuBackend()


# ---- the statement against itself
def test_the_statement_keeps_its_facts():
    pc.check_statement()


def test_the_saturated_locus_meets_its_conditions():
    pc.check_saturated_statement()


# ---- the kernels
def test_score_kernel_equals_the_dp(emu):
    pc.check_kernel(emu)


def test_banded_score_kernel_equals_the_banded_dp(emu):
    pc.check_banded_kernel(emu)


def test_two_passes_return_the_full_scores(emu):
    pc.check_two_pass(emu)


def test_refusals(emu):
    pc.check_refusals(emu)


def test_tables_feed_the_trees_unchanged(emu):
    pc.check_trees(emu)


# ---- whole MSAs
def test_the_saturated_locus(emu):
    pc.check_saturated(emu)


def test_msas_equal_the_statement(emu):
    pc.check_msas(emu)


def test_band_device_tree_and_small_budgets_give_the_same_bytes(emu):
    pc.check_same_bytes(emu)


def test_adjust_direction(emu):
    pc.check_adjust_direction(emu)


def test_collapse(emu):
    pc.check_collapse(emu)


def test_large_loci(emu):
    pc.check_large_loci(emu)


def test_seq_weights(emu):
    pc.check_seq_weights(emu)


def test_pair_scores_are_computed_once(emu):
    pc.check_pairs_once(emu)


def test_retree_refine_tree_and_refine_after_it(emu):
    pc.check_after(emu)


def test_a_locus_above_the_cap(emu):
    pc.check_cap(emu)


def test_what_moves_between_host_and_device(emu):
    pc.check_trace(emu)


def test_parameters(emu):
    pc.check_parameters(emu)


def test_the_counters_the_command_line_logs(emu):
    pc.check_cli_counts(emu)


# ---- the parser
def test_parser(capsys):
    from make_prg_amd.__main__ import main
    for argv in (["--unaligned", "--pair-distances"], ["--pair-distances"], ["--unaligned", "--band", "--pair-distances"]):
        with pytest.raises(SystemExit) as exc:
            main(["from_msa", "-i", "d", "-o", "o"] + argv)
        assert exc.value.code == 2 and "--pair-distances needs --progressive" in capsys.readouterr().err
