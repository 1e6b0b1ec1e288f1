"""Progressive MSAs past 4 096 records, `from_msa --unaligned --progressive --collapse-identical --large-loci`
(make_prg_amd/from_msa/star_align.py "Large loci", csrc/k_prog_tree_wide.inc), on the CPU emulation build: mprg_prog_tree_wide against
mprg_prog_tree, the spec's plain statements and the host's tree, scale invariance, exactness where float64 quotients tie and where
the cross products leave 64 bits, the limit and the refusals; whole MSAs of thousands of records over a dozen alleles against
tests/large_ref.py, the compositions, the limits by parameter, what moves between host and device, and the parser
(tests/large_common.py holds the checks)."""
import pytest

from tests import large_common as lc
from tests.emu.backend import EmuBackend


@pytest.fixture(scope="module")
def emu():
    return EmuBackend()


@pytest.mark.parametrize("weighted", [False, True])
def test_same_trees_below_the_old_limit(emu, weighted):
    lc.check_same_below_limit(emu, weighted)


def test_scale_invariance_across_the_old_limit(emu):
    lc.check_scale_invariance(emu)


def test_exact_where_float64_quotients_tie(emu):
    lc.check_exact(emu)


def test_products_that_leave_64_bits(emu):
    lc.check_overflow(emu)


def test_limit_and_refusals(emu):
    lc.check_refusals(emu)


def test_prog_trees_routes_by_weight_sum(emu):
    lc.check_prog_trees(emu)


def test_bytes_and_counters(emu):
    lc.check_bytes_and_counters(emu)


def test_device_tree_band_and_budget_groups(emu):
    lc.check_compositions(emu)


def test_adjust_direction(emu):
    lc.check_adjust_direction(emu)


def test_refine_tree(emu):
    lc.check_refine_tree(emu)


def test_refine(emu):
    lc.check_refine(emu)


def test_limits_by_parameter(emu):
    lc.check_limits(emu)


def test_what_moves_between_host_and_device(emu):
    lc.check_trace(emu)


def test_large_loci_needs_progressive_and_collapse(emu, capsys):
    from make_prg_amd.__main__ import main
    for argv, needs in ((["--unaligned", "--large-loci"], "--progressive"), (["--unaligned", "--collapse-identical", "--large-loci"], "--progressive"),
                        (["--unaligned", "--progressive", "--large-loci"], "--collapse-identical"),
                        (["--unaligned", "--progressive", "--device-tree", "--large-loci"], "--collapse-identical")):
        with pytest.raises(SystemExit) as exc:
            main(["from_msa", "-i", "d", "-o", "o"] + argv)
        assert exc.value.code == 2 and f"--large-loci needs {needs}" in capsys.readouterr().err
    lc.check_parameters(emu)
