"""Sequence weights, `from_msa --unaligned --progressive --seq-weights`, on the CPU emulation build: mprg_prog_leaf_weights against the
plain statement on hand-written tables, its refusals, whole MSAs against tests/weights_ref.py, the compositions with the other
flags, what moves between host and device, and the parser (tests/weights_common.py holds the checks)."""
import pytest

from tests import weights_common as wc


@pytest.fixture(scope="module")
def backend():
    from tests.emu.backend import EmuBackend
    return EmuBackend()


def test_kernel_equals_the_plain_statement(backend):
    wc.check_kernel(backend)


def test_all_distances_zero_and_all_distances_largest(backend):
    wc.check_extremes(backend)


def test_multiplicities_up_to_two_to_the_twenty(backend):
    wc.check_heavy(backend)


def test_four_thousand_and_ninety_six_leaves(backend):
    wc.check_most_leaves(backend)


def test_refusals(backend):
    wc.check_refusals(backend)


def test_msas_equal_the_statement(backend):
    wc.check_msas(backend)


def test_band_device_tree_and_small_budgets_give_the_same_bytes(backend):
    wc.check_same_bytes(backend)


def test_flag_off_is_today_s_bytes_and_trace(backend):
    wc.check_flag_off(backend)


def test_a_constant_factor_on_the_weights_changes_nothing(backend):
    wc.check_scaling(backend)


def test_over_sampled_loci(backend):
    wc.check_oversampled(backend)


def test_collapse(backend):
    wc.check_collapse(backend)


def test_large_loci(backend):
    wc.check_large_loci(backend)


def test_adjust_direction(backend):
    wc.check_adjust_direction(backend)


def test_retree_refine_tree_and_refine(backend):
    wc.check_retree_and_refine_tree(backend)


def test_what_moves_between_host_and_device(backend):
    wc.check_trace(backend)


def test_parameters(backend):
    wc.check_parameters(backend)


# ---- the parser
def test_parser(capsys):
    from make_prg_amd.__main__ import main
    for argv in (["--unaligned", "--seq-weights"], ["--seq-weights"], ["--unaligned", "--band", "--seq-weights"]):
        with pytest.raises(SystemExit) as exc:
            main(["from_msa", "-i", "d", "-o", "o"] + argv)
        assert exc.value.code == 2 and "--seq-weights needs --progressive" in capsys.readouterr().err
