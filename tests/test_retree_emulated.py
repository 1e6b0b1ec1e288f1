"""Retree, `from_msa --unaligned --progressive --retree` (make_prg_amd/from_msa/star_align.py "Retree", csrc/k_prog_retree.inc), on
the CPU emulation build: the plain-Python statement against itself, mprg_prog_identities called directly (shapes, offsets,
permuted leaves, poisoned tables, refusals), its tables through the tree entry points, whole MSAs against the statement, the
compositions with the other flags, what moves between host and device, and the parser (tests/retree_common.py holds the checks)."""
import pytest

from make_prg_amd.from_msa import star_align as sa
from tests import prog_ref as pr
from tests import refine_ref as rr
from tests import retree_common as rc
from tests import retree_ref as rt
from tests import treerefine_ref as tf
from tests.emu.backend import EmuBackend


@pytest.fixture(scope="module")
def emu():
    return EmuBackend()


# ---- the statement against itself
def test_identities_count_equal_bases_only():
    rows = ["AC-GTNRA", "AC-GANRC", "--------", "NNNNNNNN", "ACTGTNYA"]
    s, nw = rt.identities(rows)
    assert nw == [5, 5, 0, 0, 6] and s[0][1] == 3 and s[0][4] == 5 and s[1][4] == 3
    assert s[0][2] == s[0][3] == s[2][3] == s[2][2] == 0            # '-' against '-', N against N and R against R are no match
    D = rt.distances([4, 0, 7, 9, 2], rows)
    assert D[4][0] == (1 << 16) - ((1 << 16) * 3) // 5 and D[4][2] == (1 << 16) - (1 << 16) * 5 // 5 == 0 and D[7][9] == D[4][7] == 1 << 16
    assert all(D[a][b] == D[b][a] and D[a][a] == 0 for a in D for b in D)


def test_no_rebuild_gives_the_progressive_rows():
    for l in pr.table_loci()[::7] + rr.special_loci():
        rows, info, prog, _, _ = rt.progressive(l, 0)
        assert rows == pr.progressive_rows(l) and prog == pr.progressive(l)[1]
        assert info[:3] == (0, 0, None) and info[3] == info[4] == rr.objective(rows)


def test_the_statement_keeps_its_promises():
    rc.check_counts()
    for l, (rows, info, _, _, _) in zip(rc.msa_loci(), rc.msa_spec()):
        rc.invariants(l, rows)
        assert info[4] >= info[3] and info[4] == rr.objective(rows)
        if not info[1]:
            assert rows == pr.progressive_rows(l)


def test_the_constants_are_the_module_s():
    assert rt.SCALE == sa.PROG_SCALE and rt.MAX_REBUILDS == sa.RETREE_MAX and sa.RETREE_DEFAULT == 1
    assert tf.objective(["AC", "A-"]) == rr.objective(["AC", "A-"])


# ---- the kernel
def test_kernel_equals_the_plain_statement(emu):
    rc.check_kernel(emu)


def test_refusals(emu):
    rc.check_refusals(emu)


def test_tables_feed_the_tree_unchanged(emu):
    rc.check_trees(emu)


# ---- whole MSAs
def test_msas_equal_the_statement(emu):
    rc.check_msas(emu)


def test_one_rebuild(emu):
    rc.check_one_rebuild(emu)


def test_band_device_tree_and_small_budgets_give_the_same_bytes(emu):
    rc.check_same_bytes(emu)


def test_adjust_direction(emu):
    rc.check_adjust_direction(emu)


def test_collapse(emu):
    rc.check_collapse(emu)


def test_large_loci(emu):
    rc.check_large_loci(emu)


def test_refine_tree_and_refine_after_it(emu):
    rc.check_refine_after(emu)


def test_a_merge_beyond_the_limit_ends_the_locus_s_retree(emu):
    rc.check_limit(emu)


def test_what_moves_between_host_and_device(emu):
    rc.check_trace(emu)


def test_parameters(emu):
    rc.check_parameters(emu)


def test_the_counters_the_command_line_logs(emu):
    rc.check_cli_counts(emu)


# ---- the parser
def test_parser(capsys):
    from make_prg_amd.__main__ import main
    for argv, text in ((["--unaligned", "--retree"], "--retree needs --progressive"),
                       (["--retree", "2"], "--retree needs --progressive"),
                       (["--unaligned", "--progressive", "--retree", "0"], "--retree takes 1 to 4 rebuilds"),
                       (["--unaligned", "--progressive", "--retree", "5"], "--retree takes 1 to 4 rebuilds")):
        with pytest.raises(SystemExit) as exc:
            main(["from_msa", "-i", "d", "-o", "o"] + argv)
        assert exc.value.code == 2 and text in capsys.readouterr().err
