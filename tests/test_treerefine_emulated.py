"""Tree refinement, `from_msa --unaligned --progressive --refine-tree` (make_prg_amd/from_msa/star_align.py "Tree refinement",
csrc/k_tree_refine.inc), on the CPU emulation build: the plain-Python statement against itself, mprg_tree_split and
mprg_tree_objective called directly, whole MSAs against the statement (one and two passes; --band, --device-tree and a small
budget: the same bytes), --collapse-identical, the cap, the compositions with --adjust-direction and --refine, the flag off, and
the parser (tests/treerefine_common.py holds the checks)."""
import pytest

from make_prg_amd.from_msa import star_align as sa
from tests import collapse_ref as cr
from tests import prog_ref as pr
from tests import refine_ref as rr
from tests import treerefine_common as tc
from tests import treerefine_ref as tr
from tests.emu.backend import EmuBackend


@pytest.fixture(scope="module")
def emu():
    return EmuBackend()


# ---- the statement against itself
def test_weighted_objective_is_the_expanded_rows_objective():
    rows = ["AC-GT-A", "ACNGTTA", "A--GT-A", "-CRG--A"]
    for w, e in (([1, 1, 1, 1], 0), ([3, 1, 2, 5], 0), ([2, 4, 1, 1], 3)):
        want = rr.objective(cr.expanded(rows, w) + ["-" * 7] * e)
        assert tr.objective(rows, w, e) == want == rr.objective_by_pairs(cr.expanded(rows, w) + ["-" * 7] * e)
    assert tr.objective(rows) == rr.objective(rows)


def test_steps_of_a_caterpillar_and_of_a_balanced_tree():
    # a caterpillar over 6 leaves: node t holds leaves 0 .. t + 1; nodes 0 .. 2 leave two leaves or more outside
    cat = [(0, 1), (0, 2), (0, 3), (0, 4), (0, 5)]
    assert tr.steps(cat) == [[0, 1], [0, 1, 2], [0, 1, 2, 3]]
    # balanced over 8: four cherries, two nodes of four, the root; the root's children (nodes 4 and 5) cut one split: 4 is left out
    bal = [(0, 1), (2, 3), (4, 5), (6, 7), (0, 2), (4, 6), (0, 4)]
    assert tr.steps(bal) == [[0, 1], [2, 3], [4, 5], [6, 7], [4, 5, 6, 7]]
    # the root's children are a leaf and an inner node: nothing is left out, the inner child's split leaves one leaf and is no step
    assert tr.steps([(1, 2), (3, 4), (1, 3), (0, 1)]) == [[1, 2], [3, 4]]
    assert tr.steps([(0, 1), (0, 2)]) == [] and tr.steps([(0, 1)]) == [] and tr.steps([]) == []
    for merges in (cat, bal, [(1, 2), (3, 4), (1, 3), (0, 1)], [(0, 1), (0, 2)], [(0, 1)], []):
        assert [g.tolist() for g in sa.tree_steps(merges)] == tr.steps(merges)


def test_merge_order_is_the_tree_prog_ref_builds():
    for l in pr.table_loci()[::5]:
        D = pr.distances(l)[0]
        merges, tree = tr.merge_order(D, list(range(len(l))))
        assert tree == pr.upgma(D, list(range(len(l)))) and len(merges) == len(l) - 1


def test_no_pass_gives_the_progressive_rows():
    for l in pr.table_loci()[::7] + rr.special_loci():
        rows, info = tr.progressive(l, 0)
        assert rows == pr.progressive_rows(l) and info[:3] == (0, 0, 0) and info[3] == info[4] == rr.objective(rows)


def test_split_keeps_order_and_drops_all_gap_columns():
    assert tr.split(["A-C-", "-G--", "A--T", "----"], [0, 1, 0, 1]) == (["AC-", "A-T"], ["G", "-"])


def test_table_loci_accept_and_refuse():
    tc.check_counts()


# ---- the kernels, called directly
def test_split_equals_numpy(emu):
    tc.check_split(emu)


def test_split_statuses(emu):
    tc.check_split_statuses(emu)


def test_objective_equals_the_expanded_text(emu):
    tc.check_objective(emu)


def test_objective_statuses(emu):
    tc.check_objective_statuses(emu)


# ---- whole MSAs
@pytest.mark.parametrize("passes", [1, 2])
def test_msas_equal_the_spec(emu, passes):
    tc.check_msas(emu, passes)


def test_band_gives_the_same_bytes(emu):
    tc.check_same_bytes(emu, band=True)


def test_device_tree_gives_the_same_bytes(emu):
    tc.check_same_bytes(emu, device_tree=True)


def test_small_budget_gives_the_same_bytes(emu):
    tc.check_same_bytes(emu, **tc.SMALL_BUDGET)


def test_collapse(emu):
    tc.check_collapse(emu)


def test_cap(emu):
    tc.check_cap(emu)


def test_adjust_direction_and_refine(emu):
    tc.check_compositions(emu)


def test_flag_off(emu):
    tc.check_flag_off(emu)


def test_steps_beyond_the_limit_are_skipped(emu, monkeypatch):
    """The limit itself, then a limit no step passes (no progressive merge could run under such a budget, so the rule is replaced):
    every step skipped and reported, one pass only, the progressive bytes."""
    import numpy as np
    from tests import prog_common as pc
    words = sa.pa.workspace_words(200, 300)
    assert sa._tree_step_fits(np.array([200, 200, 257]), np.array([300, 310, 300]), words).tolist() == [True, False, False]
    assert sa._tree_step_fits(np.array([1, 1, 499_999]), np.array([999_998, 999_999, 500_001]), 1 << 40).tolist() == [True, False, False]
    loci = pr.table_loci()[12:14]
    info = []
    monkeypatch.setattr(sa, "_tree_step_fits", lambda WX, WY, budget_words: np.zeros(len(WX), bool))
    msas = sa.star_msas(emu, [pc.records(l) for l in loci], progressive=True, refine_tree=2, tree_refinement=info)
    assert [m.rows_as_strings() for m in msas] == [pr.progressive_rows(l) for l in loci]
    assert all(t == s == 15 and a == 0 and s0 == s1 for t, a, s, s0, s1 in info)


def test_parser(emu, capsys):
    from make_prg_amd.__main__ import main
    for argv, text in ((["--unaligned", "--refine-tree"], "--refine-tree needs --progressive"),
                       (["--refine-tree", "2"], "--refine-tree needs --progressive"),
                       (["--unaligned", "--progressive", "--refine-tree", "0"], "--refine-tree takes 1 to 4 passes"),
                       (["--unaligned", "--progressive", "--refine-tree", "5"], "--refine-tree takes 1 to 4 passes")):
        with pytest.raises(SystemExit) as exc:
            main(["from_msa", "-i", "d", "-o", "o"] + argv)
        assert exc.value.code == 2 and text in capsys.readouterr().err
    with pytest.raises(ValueError, match="refine_tree"):
        sa.star_msas(emu, [[("a", "ACGT")]], refine_tree=1)
    for n in (0, 5, True):
        with pytest.raises(ValueError, match="refine_tree"):
            sa.star_msas(emu, [[("a", "ACGT")]], progressive=True, refine_tree=n)
