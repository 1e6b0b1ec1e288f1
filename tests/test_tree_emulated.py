"""The guide tree on the device, `from_msa --unaligned --progressive --device-tree` (make_prg_amd/from_msa/star_align.py "Progressive":
Tree, csrc/k_prog_tree.inc), on the CPU emulation build: mprg_prog_tree against the spec's plain statements and the host's tree,
the edges of the kernel's own structure, exactness where float64 quotients tie, the limit and the refusals, whole MSAs against the
flag-off run, what moves between host and device, and the parser (tests/tree_common.py holds the checks)."""
import pytest

from make_prg_amd.from_msa import star_align as sa
from make_prg_amd.update import profile_align as pa
from tests import tree_common as tc
from tests.emu.backend import EmuBackend


@pytest.fixture(scope="module")
def emu():
    return EmuBackend()


def test_small_trees_equal_the_plain_statement(emu):
    tc.check_small(emu)


def test_edges_equal_the_host_tree(emu):
    tc.check_edges(emu)


def test_weighted_edges_equal_the_host_tree(emu):
    tc.check_edges(emu, weighted=True)


def test_edges_in_budget_groups(emu):
    tc.check_edges_in_groups(emu)


def test_trees_from_sequences(emu):
    tc.check_prog_trees(emu)


def test_exact_where_float64_quotients_tie(emu):
    tc.check_exact(emu)


def test_limit_and_refusals(emu):
    tc.check_refusals(emu)


def test_msas_equal_the_flag_off_run(emu):
    tc.check_msas(emu)


def test_msas_with_a_small_budget(emu):
    tc.check_msas(emu, budget_bytes=4 * pa.workspace_words(420, 420), chunk_bytes=1 << 14)


def test_adjust_direction_refine_and_band(emu):
    tc.check_compositions(emu)


def test_collapse_gives_the_weighted_tree(emu):
    tc.check_collapse(emu)


def test_what_moves_between_host_and_device(emu):
    tc.check_trace(emu)


def test_device_tree_needs_progressive(emu, capsys):
    from make_prg_amd.__main__ import main
    for argv in (["--device-tree"], ["--unaligned", "--device-tree"], ["--unaligned", "--band", "--device-tree"]):
        with pytest.raises(SystemExit) as exc:
            main(["from_msa", "-i", "d", "-o", "o"] + argv)
        assert exc.value.code == 2 and "--device-tree needs --progressive" in capsys.readouterr().err
    with pytest.raises(ValueError, match="device_tree"):
        sa.star_msas(emu, [[("a", "ACGT")]], device_tree=True)
